// verify.hip — the tail of a speculative verify pass (gemma_engine_verify, DESIGN.md §5b‴): the
// accept rule and the advance over the accepted prefix in one launch, then the rejected rows' K / V
// cleared.  Both read the accepted count from device memory: no host round trip inside the pass.
#include "kernels.h"
#include "pick.h"

namespace ghip {
namespace {

// Row i of the pass (i <= k) picked g_i for sequence index p0 + i + 1 (its n_parts partial argmax
// keys, or the sampler's one key); hist[p0 + 1 + i] holds draft[i] (i < k).  a = the number of
// leading drafts that equal their row's pick.  Then what a + 1 calls of k_advance leave: hist, the
// token, the position, its RoPE row with the position word, one epoch bump.
__global__ void __launch_bounds__(256) k_verify_accept(verify_args v) {
    __shared__ unsigned long long red[4];
    __shared__ int gs[GEMM_SKINNY_MAX_T], a_sh;
    const int tid = threadIdx.x;
    for (int i = 0; i <= v.k; ++i) {
        const unsigned long long best = block_max_key(v.keys + (int64_t)i * v.key_stride, v.n_parts, red);
        if (tid == 0) gs[i] = key_index(best);
        __syncthreads();  // red[] is reused by the next row: thread 0 has read it
    }
    if (tid == 0) {
        int a = 0;
        while (a < v.k && v.hist[v.p0 + 1 + a] == gs[a]) ++a;  // stops at the first mismatch
        for (int i = 0; i <= a; ++i) v.hist[v.p0 + 1 + i] = gs[i];
        for (int i = a + 1; i < v.k; ++i) v.hist[v.p0 + 1 + i] = 0;  // the rejected drafts behind them
        *v.token = gs[a];
        *v.pos = v.p0 + a + 1;
        if (v.r.epoch) ++*v.r.epoch;
        v.out[0] = a;
        for (int i = 0; i <= v.k; ++i) v.out[1 + i] = gs[i];
        a_sh = a;
    }
    __syncthreads();
    const int p = v.p0 + a_sh + 1;
    if (v.r.cur && p < v.r.ctx) publish_rope_row(v.r.cur, v.r.cos, v.r.sin, v.r.half, p);
    for (int j = tid; j < v.n_zero; j += 256) v.zero_keys[j] = 0;
}

// K rows and V columns p0 + a + 1 .. p0 + k of layer blockIdx.x (the rows the pass stored under
// rejected drafts) back to zero; a = *accepted
__global__ void __launch_bounds__(256) k_verify_clean(uint16_t *kc, uint16_t *vc, int64_t layer_stride, int ctx, int kvw,
                                                      int p0, int k, const int *accepted) {
    const int a = *accepted, r0 = p0 + a + 1, n = k - a;
    uint16_t *K = kc + (int64_t)blockIdx.x * layer_stride, *V = vc + (int64_t)blockIdx.x * layer_stride;
    for (int idx = threadIdx.x; idx < n * kvw; idx += 256) {
        const int r = r0 + idx / kvw, j = idx % kvw;
        K[(int64_t)r * kvw + j] = 0;
        V[(int64_t)j * ctx + r] = 0;
    }
}

}  // namespace

int launch_verify_accept(const verify_args &v, hipStream_t s) {
    if (v.k < 1 || v.k >= GEMM_SKINNY_MAX_T || v.p0 < 0 || v.p0 + v.k + 1 >= v.r.ctx) {
        set_error("verify_accept: bad draft count or position");
        return -1;
    }
    hipLaunchKernelGGL(k_verify_accept, dim3(1), dim3(256), 0, s, v);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_verify_clean(uint16_t *kc, uint16_t *vc, int n_layer, int64_t layer_stride, int ctx, int kvw, int p0, int k,
                        const int *accepted, hipStream_t s) {
    if (p0 < 0 || k < 1 || p0 + k >= ctx) {
        set_error("verify_clean: rows outside the cache");
        return -1;
    }
    hipLaunchKernelGGL(k_verify_clean, dim3(n_layer), dim3(256), 0, s, kc, vc, layer_stride, ctx, kvw, p0, k, accepted);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
