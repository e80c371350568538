// sample_full.hip — seeded temperature / top-p sampling over every entry of a logits row, nothing
// sorted (DESIGN.md §5b″ "The whole vocabulary"; the rule: include/gemma_hpc.h at GEMMA_TOP_K_ALL).
//
// Every logit gets an integer mass q_i = floor(exp((l_i - l_max) / T) * 2^40); after that exp all is
// u64 arithmetic, so sums do not depend on the order atomics arrive in.  The nucleus is a threshold
// on the sampler's monotone u32 key, found by a radix descent over mass histograms (12 + 10 + 10 key
// bits); the draw walks prefix sums in index order: over chunks of 2048 indices, then inside one chunk.
// Six launches, kernel boundaries the only ordering between workgroups (grid.y = the row):
//   k_full_max     wide: the row's maximum key, one atomicMax per workgroup
//   k_full_mass    wide: q_i of every entry into the row's q scratch (sample_ws::list_b, idle for such
//                  a row) and into an LDS mass histogram over the key's top 12 bits, flushed with u64 atomics
//   k_full_refine  wide, twice: every workgroup rescans the finished histograms for the boundary bin of
//                  each finished level, then adds the q_i of the entries that share that key prefix into
//                  the next level's 1024 bins (top_p == 1: both return after reading the parameters)
//   k_full_blocks  wide: the threshold key from the three histograms; per chunk of 2048 indices the
//                  kept mass and the kept count, plain stores to the chunk's own slot
//   k_full_pick    one workgroup of 1024: a scan of the chunk masses gives M, r and r's chunk; a scan
//                  of that chunk's 2048 masked masses gives the token; one argmax-format key for
//                  k_advance; the max word and the histograms back to zero for the next call
// A workgroup of the wide kernels owns chunks blockIdx.x, + gridDim.x, ...: 256 threads x 8 indices,
// the truncated sampler's mapping.  A row whose parameters do not ask for this sampler leaves every
// kernel on a wave-uniform branch before its first barrier or atomic.
#include <algorithm>

#include "sample_impl.h"

namespace ghip {
namespace {

typedef unsigned long long u64;
constexpr int SF_PICK = 1024;  // k_full_pick's workgroup: two entries of a chunk per thread
constexpr int SF_B1 = 4096, SF_BN = 1024;  // bins of the first level, of the two below it
static_assert(SF_PICK * 2 == SM_CHUNK && SF_B1 == 16 * SM_TH && SAMPLE_FULL_H2 - SAMPLE_FULL_H1 == SF_B1 &&
              SAMPLE_FULL_H3 - SAMPLE_FULL_H2 == SF_BN && SAMPLE_FULL_HDR - SAMPLE_FULL_H3 == SF_BN &&
              SAMPLE_FULL_MAX_V / SM_CHUNK <= 4 * SF_PICK && SF_PICK == SAMPLE_MAX_K, "whole-vocabulary sampler geometry");

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// A finished mass histogram seen from the top bin down by a workgroup of NW waves: thread t owns bins
// 16t .. 16t + 15 (threads past the histogram own none); sum = their mass, above = the mass of every
// higher bin, total = the histogram's.  wtot: NW u64 of LDS.  Two barriers.
struct hist_view {
    u64 loc[16], sum, above, total;
};
template <int NW>
__device__ __forceinline__ void view_hist(const u64 *h, int nbins, u64 *wtot, hist_view &o) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool own = tid * 16 < nbins;
    o.sum = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        ulonglong2 v = make_ulonglong2(0, 0);
        if (own) v = *(const ulonglong2 *)(h + tid * 16 + q * 2);
        o.loc[2 * q] = v.x; o.loc[2 * q + 1] = v.y;
        o.sum += v.x + v.y;
    }
    u64 incl = o.sum;  // this thread's bins and those of the wave's higher threads
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 v = __shfl_down(incl, off);
        if (lane + off < 64) incl += v;
    }
    if (lane == 0) wtot[wave] = incl;
    __syncthreads();
    o.above = incl - o.sum;
    o.total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const u64 t = wtot[w];
        o.total += t;
        if (w > wave) o.above += t;
    }
    __syncthreads();
}
// the largest bin b with (mass of bins >= b) >= target, and the mass above it, into res[0], res[1]
// (LDS; {0, 0} when target is outside [1, total]).  Two barriers.
__device__ __forceinline__ void cut_bin(const hist_view &o, u64 target, u64 *res) {
    if (threadIdx.x == 0) res[0] = res[1] = 0;
    __syncthreads();
    if (o.above < target && target <= o.above + o.sum) {  // exactly one thread
        u64 a = o.above;
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (a + o.loc[j] >= target) {
                res[0] = (u64)(threadIdx.x * 16 + j);
                res[1] = a;
                break;
            }
            a += o.loc[j];
        }
    }
    __syncthreads();
}
// The threshold key's leading `levels` digits (12, 10, 10 bits) from the row's finished histograms,
// the lower digits 0: after three levels the threshold key itself, the largest key value whose
// entries and all above them hold at least P = max((u64)(top_p * W), 1) of the mass W.  top_p == 1:
// 0, every entry is kept, nothing is read.  Every thread of the workgroup calls it; lds: NW + 6 u64.
template <int NW>
__device__ __forceinline__ uint32_t threshold_key(const sampler_params &P, const u64 *ws, int levels, u64 *lds) {
    if (P.top_p == 1.0f) return 0;
    u64 *wtot = lds, *res = lds + NW;
    hist_view o;
    view_hist<NW>(ws + SAMPLE_FULL_H1, SF_B1, wtot, o);
    u64 target = (u64)((double)P.top_p * (double)o.total);
    if (target < 1) target = 1;
    cut_bin(o, target, res);
    uint32_t theta = (uint32_t)res[0] << 20;
    if (levels < 2) return theta;
    target -= res[1];
    view_hist<NW>(ws + SAMPLE_FULL_H2, SF_BN, wtot, o);
    cut_bin(o, target, res + 2);
    theta |= (uint32_t)res[2] << 10;
    if (levels < 3) return theta;
    target -= res[3];
    view_hist<NW>(ws + SAMPLE_FULL_H3, SF_BN, wtot, o);
    cut_bin(o, target, res + 4);
    return theta | (uint32_t)res[4];
}

// every thread's v summed over a workgroup of NW waves: the sum of the lower threads' (returned) and
// the total.  wtot: NW u64 of LDS.  Two barriers.
template <int NW>
__device__ __forceinline__ u64 block_prefix(u64 v, u64 *wtot, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    u64 pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const u64 t = wtot[w];
        tot += t;
        if (w < wave) pre += t;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

// LDS bins added to the row's global histogram: non-zero bins only, u64 integer atomics
__device__ __forceinline__ void flush_bins(const u64 *h, int nbins, u64 *gh) {
    for (int i = threadIdx.x; i < nbins; i += SM_TH) {
        const u64 c = h[i];
        if (c) atomicAdd(&gh[i], c);
    }
}

__global__ void __launch_bounds__(SM_TH) k_full_max(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                    const slot_row *tab, u64 *ws, int64_t stride) {
    __shared__ unsigned red[SM_TH / 64];
    const sampler_params P = row_params(prm, tab);
    if (!samples_full(P)) return;
    const int tid = threadIdx.x;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    unsigned m = 0;
    for (int64_t base = (int64_t)blockIdx.x * SM_CHUNK; base < n; base += (int64_t)gridDim.x * SM_CHUNK) {
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = base + k * SM_TH + tid;
            if (i < n) m = max(m, logit_key(row[i]));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor(m, off));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SM_TH / 64; ++w) m = max(m, red[w]);
        atomicMax((unsigned *)(ws + (int64_t)blockIdx.y * stride), m);  // the max word's low half
    }
}

__global__ void __launch_bounds__(SM_TH) k_full_mass(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                     const slot_row *tab, u64 *ws, int64_t stride, u64 *qs, int64_t cap_q) {
    __shared__ u64 h[SF_B1];
    const sampler_params P = row_params(prm, tab);
    if (!samples_full(P)) return;
    const int tid = threadIdx.x;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    ws += (int64_t)blockIdx.y * stride;
    qs += (int64_t)blockIdx.y * cap_q;
    for (int i = tid; i < SF_B1; i += SM_TH) h[i] = 0;
    __syncthreads();
    const double l_max = (double)__builtin_bit_cast(float, unordered_bits((uint32_t)ws[0]));
    const double temp = (double)P.temperature;
    for (int64_t base = (int64_t)blockIdx.x * SM_CHUNK; base < n; base += (int64_t)gridDim.x * SM_CHUNK) {
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = base + k * SM_TH + tid;
            if (i < n) {
                const float v = row[i];
                const u64 q = (u64)(exp(((double)v - l_max) / temp) * 0x1.0p40);  // in [0, 2^40]: the cast is the floor
                qs[i] = q;
                if (q) atomicAdd(&h[logit_key(v) >> 20], q);
            }
        }
    }
    __syncthreads();
    flush_bins(h, SF_B1, ws + SAMPLE_FULL_H1);
}

// level 1: the next 10 key bits of the entries in the first level's boundary bin; level 2: the last 10
__global__ void __launch_bounds__(SM_TH) k_full_refine(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                       const slot_row *tab, u64 *ws, int64_t stride, const u64 *qs,
                                                       int64_t cap_q, int level) {
    __shared__ u64 h[SF_BN];
    __shared__ u64 lds[SM_TH / 64 + 6];
    const sampler_params P = row_params(prm, tab);
    if (!samples_full(P) || P.top_p == 1.0f) return;
    const int tid = threadIdx.x;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    ws += (int64_t)blockIdx.y * stride;
    qs += (int64_t)blockIdx.y * cap_q;
    for (int i = tid; i < SF_BN; i += SM_TH) h[i] = 0;
    const int shift = level == 1 ? 20 : 10;
    const uint32_t prefix = threshold_key<SM_TH / 64>(P, ws, level, lds) >> shift;  // (its barriers order the zeroing)
    for (int64_t base = (int64_t)blockIdx.x * SM_CHUNK; base < n; base += (int64_t)gridDim.x * SM_CHUNK) {
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = base + k * SM_TH + tid;
            if (i < n) {
                const uint32_t key = logit_key(row[i]);
                if ((key >> shift) == prefix) {
                    const u64 q = qs[i];
                    if (q) atomicAdd(&h[(key >> (shift - 10)) & (SF_BN - 1)], q);
                }
            }
        }
    }
    __syncthreads();
    flush_bins(h, SF_BN, ws + (level == 1 ? SAMPLE_FULL_H2 : SAMPLE_FULL_H3));
}

__global__ void __launch_bounds__(SM_TH) k_full_blocks(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                       const slot_row *tab, u64 *ws, int64_t stride, const u64 *qs,
                                                       int64_t cap_q) {
    __shared__ u64 lds[SM_TH / 64 + 6];
    __shared__ u64 red[2 * (SM_TH / 64)];
    const sampler_params P = row_params(prm, tab);
    if (!samples_full(P)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    ws += (int64_t)blockIdx.y * stride;
    qs += (int64_t)blockIdx.y * cap_q;
    const uint32_t theta = threshold_key<SM_TH / 64>(P, ws, 3, lds);
    const int64_t n_chunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        u64 mass = 0, cnt = 0;
#pragma unroll
        for (int k = 0; k < SM_PER; ++k) {
            const int64_t i = c * SM_CHUNK + k * SM_TH + tid;
            // (theta == 0 keeps every entry: the logits are not read again)
            if (i < n && (theta == 0 || logit_key(row[i]) >= theta)) {
                mass += qs[i];
                ++cnt;
            }
        }
        mass = wave_sum(mass);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            red[wave] = mass;
            red[SM_TH / 64 + wave] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SM_TH / 64; ++w) {
                mass += red[w];
                cnt += red[SM_TH / 64 + w];
            }
            ws[SAMPLE_FULL_HDR + c] = mass;  // the chunk's own slots: no atomics
            ws[SAMPLE_FULL_HDR + n_chunks + c] = cnt;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SF_PICK) k_full_pick(const float *lg, int64_t ld, int64_t n, const sampler_params *prm,
                                                       const int *pos, const slot_row *tab, u64 *ws, int64_t stride,
                                                       const u64 *qs, int64_t cap_q, u64 *key_out, int key_parts,
                                                       sample_dbg dbg) {
    constexpr int NW = SF_PICK / 64;
    __shared__ u64 lds[NW + 6];
    __shared__ u64 wtot[NW];
    __shared__ u64 s_chunk, s_rest;
    __shared__ int s_j;
    const sampler_params P = row_params(prm, tab);
    if (!samples_full(P)) return;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.y;
    const float *row = lg + r * ld;
    pos = tab ? tab[r].pos : pos + r;
    ws += r * stride;
    qs += r * cap_q;
    key_out += r * key_parts;
    if (dbg.token) dbg.token += r;
    if (dbg.n_cand) dbg.n_cand += r;
    if (dbg.n_kept) dbg.n_kept += r;
    if (dbg.cand) dbg.cand[r * SAMPLE_MAX_K + tid] = -1;  // no ordered list in this mode
    const uint32_t theta = threshold_key<NW>(P, ws, 3, lds);
    // (every thread is past its reads of the histograms) scratch ready for the next call
    for (int i = tid; i < SAMPLE_FULL_HDR; i += SF_PICK) ws[i] = 0;

    // M and the chunk that holds r: thread t owns chunks t * per .. t * per + per - 1, per <= 4
    const int64_t n_chunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    const int per = (int)((n_chunks + SF_PICK - 1) / SF_PICK);
    u64 cm[4], mine = 0, kept = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t c = (int64_t)tid * per + k;
        cm[k] = 0;
        if (k < per && c < n_chunks) {
            cm[k] = ws[SAMPLE_FULL_HDR + c];
            kept += ws[SAMPLE_FULL_HDR + n_chunks + c];
        }
        mine += cm[k];
    }
    if (tid == 0) {
        s_chunk = ~0ull;
        s_j = -1;
    }
    u64 M, n_kept;
    const u64 below = block_prefix<NW>(mine, wtot, &M);
    (void)block_prefix<NW>(kept, wtot, &n_kept);
    // the histograms, the chunk slots and q agree, so the searches below find their entry; were the
    // scratch ever clobbered, never hand k_advance an index outside the row: token 0
    bool ok = M > 0;
    if (ok) {
        u64 rr = (u64)(draw_uniform(P.seed, *pos + 1) * (double)M);
        if (rr > M - 1) rr = M - 1;
        if (below <= rr && rr < below + mine) {  // exactly one thread
            u64 a = below;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (rr < a + cm[k]) {
                    s_chunk = (u64)((int64_t)tid * per + k);
                    s_rest = rr - a;
                    break;
                }
                a += cm[k];
            }
        }
    }
    __syncthreads();
    const u64 chunk = s_chunk;
    ok = ok && chunk < (u64)n_chunks;
    if (ok) {
        // that chunk's 2048 entries in index order, two per thread, masked by the threshold
        const u64 rest = s_rest;
        const int64_t i0 = (int64_t)chunk * SM_CHUNK + 2 * tid;
        u64 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t i = i0 + k;
            v[k] = i < n && (theta == 0 || logit_key(row[i]) >= theta) ? qs[i] : 0;
        }
        u64 total;
        const u64 before = block_prefix<NW>(v[0] + v[1], wtot, &total);
        if (before <= rest && rest < before + v[0] + v[1]) s_j = (int)(rest < before + v[0] ? i0 : i0 + 1);  // its mass is > 0: i < n
        __syncthreads();
    }
    const int j = ok ? s_j : -1;
    const u64 pick = j >= 0 ? pack_key(logit_key(row[j]), j) : 0x80000000FFFFFFFFull;
    // (key_parts > 1: the rest of the row's partial keys become key 0, below every candidate)
    if (tid < key_parts) key_out[tid] = tid == 0 ? pick : 0ull;
    if (tid == 0) {
        if (dbg.token) *dbg.token = key_index(pick);
        if (dbg.n_cand) *dbg.n_cand = (int)n;
        if (dbg.n_kept) *dbg.n_kept = (int)n_kept;
    }
}

}  // namespace

int launch_sample_full(const float *lg, int64_t ld, int rows, int64_t n, const sampler_params *prm, const int *pos,
                       const slot_row *tab, const sample_ws &w, const sample_dbg &dbg, hipStream_t s, int key_parts) {
    const int64_t n_chunks = (n + SM_CHUNK - 1) / SM_CHUNK;
    if (!w.full || n > SAMPLE_FULL_MAX_V || w.full_stride < SAMPLE_FULL_HDR + 2 * n_chunks || key_parts > SF_PICK) {
        set_error("sampler: scratch not sized for these rows");
        return -1;
    }
    const dim3 wide((unsigned)std::min<int64_t>(n_chunks, SM_GRID_MAX), rows), th(SM_TH);
    const u64 *qs = w.list_b;
    hipLaunchKernelGGL(k_full_max, wide, th, 0, s, lg, ld, n, prm, tab, w.full, w.full_stride);
    hipLaunchKernelGGL(k_full_mass, wide, th, 0, s, lg, ld, n, prm, tab, w.full, w.full_stride, w.list_b, w.cap_b);
    hipLaunchKernelGGL(k_full_refine, wide, th, 0, s, lg, ld, n, prm, tab, w.full, w.full_stride, qs, w.cap_b, 1);
    hipLaunchKernelGGL(k_full_refine, wide, th, 0, s, lg, ld, n, prm, tab, w.full, w.full_stride, qs, w.cap_b, 2);
    hipLaunchKernelGGL(k_full_blocks, wide, th, 0, s, lg, ld, n, prm, tab, w.full, w.full_stride, qs, w.cap_b);
    hipLaunchKernelGGL(k_full_pick, dim3(1, rows), dim3(SF_PICK), 0, s, lg, ld, n, prm, pos, tab, w.full, w.full_stride, qs,
                       w.cap_b, w.key, key_parts, dbg);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
