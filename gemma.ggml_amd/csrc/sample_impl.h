// sample_impl.h — what the two samplers' kernels share (device inlines only; included by sample.hip,
// the truncated sampler, and sample_full.hip, the whole-vocabulary one; DESIGN.md §5b″).
#pragma once

#include "kernels.h"
#include "pick.h"

namespace ghip {

constexpr int SM_TH = 256, SM_PER = 8, SM_CHUNK = SM_TH * SM_PER;  // logits per workgroup pass
constexpr int SM_GRID_MAX = 1024;
static_assert(SM_CHUNK == SAMPLE_FULL_CHUNK, "one chunk mapping for both samplers");

// monotone key of a logit: the argmax key's high word (pick.h) with -0 made +0
__device__ __forceinline__ uint32_t logit_key(float v) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (u == 0x80000000u) u = 0;
    return ordered_bits(u);
}

// All sampler kernels: grid.y = the row of the pass.  A row's logits are lg + row * ld and its
// workspace the row-th of each sample_ws array; the offsets are wave-uniform (scalar registers).
// the row's parameters: its table entry's, else the launch's one struct
__device__ __forceinline__ sampler_params row_params(const sampler_params *prm, const slot_row *tab) {
    return tab ? tab[blockIdx.y].smp : *prm;
}
// which sampler a row's parameters ask for: none (greedy), the truncated one, the whole-vocabulary one
__device__ __forceinline__ bool samples_full(const sampler_params &p) {
    return p.temperature > 0.0f && p.top_k == SAMPLE_TOP_K_ALL;
}
__device__ __forceinline__ bool samples_truncated(const sampler_params &p) {
    return p.temperature > 0.0f && p.top_k != SAMPLE_TOP_K_ALL;
}

__device__ __forceinline__ uint64_t splitmix64_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// u in [0, 1) of the pick at sequence index p
__device__ __forceinline__ double draw_uniform(uint64_t seed, int p) {
    const uint64_t z = seed + (uint64_t)(int64_t)(p + 1) * 0x9E3779B97F4A7C15ull;
    return (double)(splitmix64_mix(z) >> 11) * 0x1.0p-53;
}

}  // namespace ghip
