// logprob.hip — the log-probability of a token under softmax(row), for every logits row of a pass
// (DESIGN.md §5b⁗′; the rule is stated in include/gemma_hpc.h at gemma_engine_set_logprobs):
//   M = max_i l[i] (floats), S = sum_i exp((double)l[i] - (double)M), lp = ((double)l[t] - M) - log(S).
//
// Two launches, a kernel boundary between them (no in-launch cross-workgroup hand-off, as the sampler):
//   k_lse_parts   grid (G, R): workgroup g reads chunk g of row r once (LSE_CHUNK logits, one 16-byte
//                 load per thread where the row is aligned, a guarded scalar tail) and leaves its float
//                 max m_g and s_g = sum exp((double)l - (double)m_g) in parts[r][g].  It needs the row
//                 only: no token, no position.
//   k_lse_finish  grid (1, R), after the advance has settled the token: M = max_g m_g, S = sum_g
//                 s_g * exp((double)m_g - (double)M) in ascending g, then the row's sequence index q,
//                 t = hist[q] and lp[q].
// The value is a function of (row, token) alone, bit for bit: G and the chunks depend on n_vocab only,
// a thread sums its four terms in index order, a wave reduces by a fixed xor butterfly (IEEE addition
// is commutative, so every lane holds the same bits), the four waves and the G partials are added in
// index order.  max is exact and order-free.
#include "kernels.h"

namespace ghip {
namespace {

constexpr int LSE_TH = 256, LSE_PER = 4;
static_assert(LSE_CHUNK == LSE_TH * LSE_PER, "one 16-byte load per thread and chunk");

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(LSE_TH) k_lse_parts(const float *lg, int64_t ld, int n, lse_part *parts) {
    __shared__ float wm[LSE_TH / 64];
    __shared__ double wsum[LSE_TH / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = lg + (int64_t)blockIdx.y * ld;
    const int i0 = blockIdx.x * LSE_CHUNK + tid * LSE_PER;
    const float ninf = -__builtin_inff();
    float v[LSE_PER] = {ninf, ninf, ninf, ninf};  // past the row's end: contributes nothing
    if (i0 + LSE_PER <= n && ((uintptr_t)(row + i0) & 15) == 0) {
        const float4 q = *(const float4 *)(row + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < LSE_PER; ++k)
            if (i0 + k < n) v[k] = row[i0 + k];
    }
    float m = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    if (lane == 0) wm[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    double s = 0.0;
    if (m != ninf) {  // a chunk of -inf only: s = 0 (never -inf - -inf)
        const double md = (double)m;
#pragma unroll
        for (int k = 0; k < LSE_PER; ++k) s += v[k] == ninf ? 0.0 : exp((double)v[k] - md);
    }
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        lse_part p;
        p.s = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        p.m = m;
        p.pad = 0.0f;
        parts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

__global__ void __launch_bounds__(LSE_TH) k_lse_finish(lse_finish_args a) {
    __shared__ float wm[LSE_TH / 64];
    __shared__ double term[LSE_MAX_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.y;
    // the rows that count: all of them, or 0 .. *acc of a verify pass (the accepted prefix)
    const int last = a.acc ? *a.acc : a.R - 1;
    if (r > last || last >= a.R) return;
    const lse_part *parts = a.parts + (int64_t)r * a.G;
    const float ninf = -__builtin_inff();
    float m = ninf;
    for (int g = tid; g < a.G; g += LSE_TH) m = fmaxf(m, parts[g].m);
    m = wave_max(m);
    if (lane == 0) wm[wave] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    for (int g = tid; g < a.G; g += LSE_TH) {
        const lse_part p = parts[g];
        term[g] = p.m == ninf ? 0.0 : p.s * exp((double)p.m - (double)M);
    }
    __syncthreads();
    if (tid != 0) return;
    double S = 0.0;
    for (int g = 0; g < a.G; ++g) S += term[g];  // ascending g
    // the sequence index the row predicts: the slot's position after its advance, or the rows of a
    // pass of consecutive positions that ends at *pos
    const int *hist = a.hist;
    double *lp = a.lp;
    int q;
    if (a.tab) {
        const slot_row sr = a.tab[r];
        hist = sr.hist; lp = sr.lp;
        q = *sr.pos;
    } else {
        q = *a.pos - (last - r);
    }
    if (q < 1 || q > a.n_ctx) return;
    const int t = hist[q];
    if (t < 0 || t >= a.n) return;
    const float lt = a.lg[(int64_t)r * a.ld + t];
    lp[q] = ((double)lt - (double)M) - log(S);
}

}  // namespace

int lse_grid(int64_t n_vocab) { return (int)((n_vocab + LSE_CHUNK - 1) / LSE_CHUNK); }

int launch_lse_parts(const float *lg, int64_t ld, int rows, int64_t n, lse_part *parts, hipStream_t s) {
    if (!lg || !parts || rows < 1 || rows > 65535 || n < 1 || n > (int64_t)LSE_MAX_G * LSE_CHUNK) {
        set_error("logprob: rows outside [1, 65535] or n_vocab outside [1, " + std::to_string((int64_t)LSE_MAX_G * LSE_CHUNK) + "]");
        return -1;
    }
    hipLaunchKernelGGL(k_lse_parts, dim3(lse_grid(n), rows), dim3(LSE_TH), 0, s, lg, ld, (int)n, parts);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_lse_finish(const lse_finish_args &a, hipStream_t s) {
    if (!a.lg || !a.parts || a.R < 1 || a.R > 65535 || a.n < 1 || a.G != lse_grid(a.n) || a.G > LSE_MAX_G ||
        (!a.tab && (!a.pos || !a.hist || !a.lp))) {
        set_error("logprob: the finish launch's rows, partials or sequence are not set");
        return -1;
    }
    hipLaunchKernelGGL(k_lse_finish, dim3(1, a.R), dim3(LSE_TH), 0, s, a);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
