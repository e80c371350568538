// pick.h — the token pick on the device, stated once (device inlines only; included by ops.hip,
// batch.hip, verify.hip, prefill.hip, sample.hip and matvec_impl.h).
//
//  * the key: a candidate (value, index) as one u64, (ordered float << 32) | ~index.  "Larger key" is
//    larger value, then smaller index: the maximum key is the strict '>' argmax whose first maximum
//    wins (src/gemma_model.cpp:538-543).  Key 0 is below every candidate.
//  * block_max_key: the maximum key of a 256-thread workgroup, in thread 0.
//  * publish_rope_row: the [cos | sin | (int)pos] row a sequence keeps current for its attention.
//  * commit_pick: a batch slot's pick into its history, under the given-token rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ghip {

// a float's bits as a u32 that orders as the float does (-0 below +0), and back
__device__ __forceinline__ uint32_t ordered_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t unordered_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

__device__ __forceinline__ unsigned long long pack_key(uint32_t ordered, int64_t idx) {
    return ((unsigned long long)ordered << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
}
__device__ __forceinline__ unsigned long long argmax_key(float v, int64_t idx) {
    return pack_key(ordered_bits(__builtin_bit_cast(uint32_t, v)), idx);
}
__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }
__device__ __forceinline__ float key_value(unsigned long long key) {
    return __builtin_bit_cast(float, unordered_bits((uint32_t)(key >> 32)));
}
// the same value under another index
__device__ __forceinline__ unsigned long long key_with_index(unsigned long long key, int64_t idx) {
    return (key & 0xFFFFFFFF00000000ull) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
}

// the maximum over a wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long best) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    return best;
}

// The maximum of every thread's `best` over a 256-thread workgroup; the result is thread 0's return
// value only.  red: 4 u64 of LDS.  One barrier: every thread's loads and stores issued before the call
// are ordered before what thread 0 does with the result.  A caller that reduces again with the same
// red[] puts a barrier between the calls (thread 0 reads red[] after this one).
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long best, unsigned long long *red) {
    best = wave_max_key(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
    return best;
}
// ... of the n keys at keys[0 .. n)
__device__ __forceinline__ unsigned long long block_max_key(const unsigned long long *keys, int n, unsigned long long *red) {
    unsigned long long best = 0;
    for (int i = threadIdx.x; i < n; i += 256) best = keys[i] > best ? keys[i] : best;
    return block_max_key(best, red);
}

// position p's RoPE row into cur = [cos | sin | (int)p] (256 threads; cos / sin: the [ctx][half] tables)
__device__ __forceinline__ void publish_rope_row(float *cur, const float *cos, const float *sin, int half, int p) {
    for (int i = threadIdx.x; i < half; i += 256) {
        cur[i] = cos[(int64_t)p * half + i];
        cur[half + i] = sin[(int64_t)p * half + i];
    }
    if (threadIdx.x == 0) ((int *)cur)[2 * half] = p;
}

// A batch slot's pick committed at sequence index q of its history (hist_cap tokens, the first `fixed`
// of them given): a given token is never overwritten, below `fixed` the pick is replaced by hist[q].
// Returns the token that stands at q.  (The single sequence's k_advance and k_verify_accept keep their
// argmax in *token instead: another rule.)
__device__ __forceinline__ int commit_pick(int *hist, int q, int fixed, int hist_cap, int pick) {
    if (q < hist_cap) {
        if (q >= fixed) hist[q] = pick;
        else pick = hist[q];
    }
    return pick;
}

}  // namespace ghip
