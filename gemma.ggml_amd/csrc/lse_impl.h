// lse_impl.h — what the two finish kernels of the log-probability work share (device inlines only;
// included by logprob.hip and toplogprob.hip): which rows of a pass count, a row's M and S from its
// partials, the sequence index a row predicts, and the value itself.  Each rule is stated here once.
#pragma once

#include "kernels.h"

namespace ghip {

constexpr int LSE_TH = 256;  // threads of k_lse_parts, k_lse_finish and k_topn_finish

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// the last row of the pass that counts: all of them, or *acc of a verify pass (the accepted prefix);
// row r counts when r <= last < R
__device__ __forceinline__ int lse_last_row(const lse_finish_args &a) { return a.acc ? *a.acc : a.R - 1; }

// LDS of lse_merge
struct lse_merge_lds {
    float wm[LSE_TH / 64];
    double term[LSE_MAX_G];
};

// M = max_g m_g in every thread; S = sum_g s_g * exp((double)m_g - (double)M) in ascending g, thread
// 0's *S alone.  256 threads, two barriers; the second orders every thread's earlier LDS traffic too.
__device__ __forceinline__ float lse_merge(const lse_part *parts, int G, lse_merge_lds &L, double *S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float ninf = -__builtin_inff();
    float m = ninf;
    for (int g = tid; g < G; g += LSE_TH) m = fmaxf(m, parts[g].m);
    m = wave_max(m);
    if (lane == 0) L.wm[wave] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(L.wm[0], L.wm[1]), fmaxf(L.wm[2], L.wm[3]));
    for (int g = tid; g < G; g += LSE_TH) {
        const lse_part p = parts[g];
        L.term[g] = p.m == ninf ? 0.0 : p.s * exp((double)p.m - (double)M);
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += L.term[g];  // ascending g
        *S = s;
    }
    return M;
}

// the sequence row r writes to and the index q it predicts there: the slot's position after its
// advance, or the rows of a pass of consecutive positions that ends at *pos.  q outside [1, n_ctx]:
// the row writes nothing (returns false)
struct lse_target {
    const int *hist;
    double *lp;
    int32_t *alt_tok;
    double *alt_lp;
    int q;
};
__device__ __forceinline__ bool lse_target_of(const lse_finish_args &a, int r, int last, lse_target *t) {
    t->hist = a.hist; t->lp = a.lp; t->alt_tok = a.alt_tok; t->alt_lp = a.alt_lp;
    if (a.tab) {
        const slot_row sr = a.tab[r];
        t->hist = sr.hist; t->lp = sr.lp; t->alt_tok = sr.alt_tok; t->alt_lp = sr.alt_lp;
        t->q = *sr.pos;
    } else {
        t->q = *a.pos - (last - r);
    }
    return t->q >= 1 && t->q <= a.n_ctx;
}

// logprob of an entry of value lt of the row with M and S
__device__ __forceinline__ double lse_value(float lt, float M, double S) { return ((double)lt - (double)M) - log(S); }

}  // namespace ghip
