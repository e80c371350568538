// penalty.hip — repetition, presence and frequency penalties on the logits rows of a pass, on the
// device (DESIGN.md §5b″ "Penalties"; the rule is stated in include/gemma_hpc.h at
// gemma_engine_set_penalties).
//
// A row that processed sequence index p is penalised over the window W = hist[p + 1 - n .. p],
// n = min(last_n, p + 1): every token t of W that lies in [0, n_vocab), with c_t its count in W, gets
//     a = l[t] <= 0 ? l[t] * repeat : l[t] / repeat;   l'[t] = a - ((float)c_t * frequency + presence)
// each operation one f32 operation rounded to nearest.  The row is changed in place and put back:
//   k_penalty_apply    one workgroup per row.  The window goes into the LDS as u32, padded with
//                      0xFFFFFFFF to m, the power of two >= n, and is sorted ascending by a bitonic
//                      network over m.  Up to 16 waves take part, wave w owning the pairs of elements
//                      [w * C, (w + 1) * C), C = m / waves >= 128 (one wave when m <= 128): a stage
//                      whose stride stays inside C touches the wave's own elements only and needs no
//                      workgroup barrier, so the common window of 64 sorts in one wave without any and
//                      a window of 8,192 takes 15 workgroup barriers for its 91 stages.  In the sorted
//                      window element i is a run head when w[i - 1] differs; a head finds its run's
//                      end by a binary search for the upper bound of its token (at most 13 LDS reads,
//                      whatever the run length), takes a slot of the row's save list (a ballot per
//                      wave, one LDS atomic per wave), saves (token, raw bits) there and stores l'[t].
//                      The tokens of the heads are distinct, so no two lanes touch one logit.
//   k_penalty_restore  the same grid: every saved (token, raw bits) back into the row, the count zeroed.
// Between the two the unchanged pick kernels read the penalised row; after them the row is the raw
// one bit for bit (log-probabilities, logits copies).  The geometry is the row count alone: last_n,
// the parameters and the position are read on the device, so a captured graph survives their change.
// A row whose setting is off, or whose position is outside its history, leaves before its first store.
#include "kernels.h"

namespace ghip {
namespace {

constexpr int PN_TH = 1024, PN_WAVES = PN_TH / 64;
constexpr unsigned PN_PAD = 0xFFFFFFFFu;  // above every token id: sorts last, never a head in range
static_assert(PENALTY_MAX_N == 8192 && PENALTY_MAX_N % PN_TH == 0, "the window fills 32 KiB of LDS");

struct pen_row {  // what a row's workgroup reads before anything else, wave-uniformly
    float *lg;
    const int *hist;
    int p;
};
__device__ __forceinline__ pen_row row_of(const penalty_args &a, int r) {
    pen_row o;
    o.lg = a.lg + (int64_t)r * a.ld;
    o.hist = a.tab ? a.tab[r].hist : a.hist + (int64_t)r * a.hist_ld;
    o.p = a.tab ? *a.tab[r].pos : a.pos[r];
    return o;
}

__device__ __forceinline__ bool params_on(const penalty_params &P) {
    return P.last_n >= 1 && P.last_n <= PENALTY_MAX_N && !(P.repeat == 1.0f && P.presence == 0.0f && P.frequency == 0.0f);
}

// what follows a stage of the network: a workgroup barrier when the stage or the next one crosses a
// wave's elements, else the wave's own LDS operations in program order are all that is needed (they
// complete in order; the fence keeps the compiler from moving them across)
__device__ __forceinline__ void stage_sync(bool workgroup) {
    if (workgroup) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// the penalised value of raw logit l whose token occurs c times in the window
__device__ __forceinline__ float penalised(float l, int c, const penalty_params &P) {
#pragma clang fp contract(off)
    const float a = l <= 0.0f ? l * P.repeat : __fdiv_rn(l, P.repeat);
    const float cf = (float)c * P.frequency;
    const float pen = cf + P.presence;
    return a - pen;
}

__global__ void __launch_bounds__(PN_TH) k_penalty_apply(const penalty_args a, uint2 *list, unsigned *count) {
    __shared__ unsigned w[PENALTY_MAX_N];
    __shared__ unsigned s_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const penalty_params P = *a.prm;
    if (!params_on(P)) return;
    const pen_row R = row_of(a, r);
    if (R.p < 0 || R.p >= a.hist_cap) return;
    const int n = P.last_n < R.p + 1 ? P.last_n : R.p + 1;
    int m = 2;
    while (m < n) m <<= 1;
    const int *win = R.hist + (R.p + 1 - n);
    for (int i = tid; i < m; i += PN_TH) w[i] = i < n ? (unsigned)win[i] : PN_PAD;
    if (tid == 0) s_count = 0;
    __syncthreads();

    // ---- the bitonic network over m: m / 2 pairs per stage, wave `wave` of nw the pairs [wave * hp, + hp)
    const int nw = m <= 128 ? 1 : (m / 128 < PN_WAVES ? m / 128 : PN_WAVES);
    const int C = m / nw, hp = C >> 1;
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (wave < nw) {
                for (int t = lane; t < hp; t += 64) {
                    const int T = wave * hp + t;
                    const int i = ((T & ~(j - 1)) << 1) | (T & (j - 1)), l = i + j;
                    const unsigned x = w[i], y = w[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        w[i] = y;
                        w[l] = x;
                    }
                }
            }
            const int jn = j > 1 ? j >> 1 : k;  // the next stage's stride (past the last stage: the heads read anywhere)
            stage_sync(2 * j > C || 2 * jn > C || (j == 1 && k == m));
        }
    }

    // ---- run heads: count, slot, save, store
    uint2 *mine = list + (int64_t)r * PENALTY_MAX_N;
    for (int base = 0; base < m; base += PN_TH) {
        const int i = base + tid;
        unsigned v = PN_PAD;
        bool head = false;
        if (i < m) {
            v = w[i];
            head = v < (unsigned)a.n_vocab && (i == 0 || w[i - 1] != v);
        }
        int c = 0;
        if (head) {  // the first index past i whose token is larger
            int lo = i + 1, hi = m;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (w[mid] <= v) lo = mid + 1;
                else hi = mid;
            }
            c = lo - i;
        }
        const unsigned long long heads = __ballot(head);
        unsigned slot0 = 0;
        if (lane == 0 && heads) slot0 = atomicAdd(&s_count, (unsigned)__popcll(heads));
        slot0 = __shfl(slot0, 0);
        if (head) {
            const unsigned slot = slot0 + (unsigned)__popcll(heads & ((1ull << lane) - 1ull));
            const float l = R.lg[v];
            mine[slot] = make_uint2(v, __builtin_bit_cast(unsigned, l));
            R.lg[v] = penalised(l, c, P);
        }
    }
    __syncthreads();
    if (tid == 0) count[r] = s_count;
}

__global__ void __launch_bounds__(PN_TH) k_penalty_restore(const penalty_args a, const uint2 *list, unsigned *count) {
    const int tid = threadIdx.x, r = blockIdx.x;
    float *lg = a.lg + (int64_t)r * a.ld;
    const uint2 *mine = list + (int64_t)r * PENALTY_MAX_N;
    unsigned n = count[r];
    if (n > (unsigned)PENALTY_MAX_N) n = PENALTY_MAX_N;
    for (unsigned i = tid; i < n; i += PN_TH) {
        const uint2 e = mine[i];
        if (e.x < (unsigned)a.n_vocab) lg[e.x] = __builtin_bit_cast(float, e.y);
    }
    __syncthreads();  // every thread has read the count
    if (tid == 0 && n) count[r] = 0;
}

bool args_ok(const penalty_args &a, const penalty_ws &w) {
    if (w.list && w.count && a.lg && a.prm && a.rows >= 1 && a.rows <= w.rows && a.n_vocab >= 1 && a.hist_cap >= 1 &&
        (a.tab || (a.pos && a.hist)))
        return true;
    set_error("penalties: no workspace for a pass of " + std::to_string(a.rows) + " rows, or no history");
    return false;
}

}  // namespace

int penalty_ws_alloc(dev_pool &mem, penalty_ws *w, hipStream_t s, int rows) {
    *w = penalty_ws{};
    if (rows < 1) {
        set_error("penalties: rows out of range");
        return -1;
    }
    if (mem.get(&w->list, (size_t)rows * PENALTY_MAX_N * sizeof(uint2)) || mem.get_zeroed(&w->count, (size_t)rows * 4, s)) {
        penalty_ws_free(mem, w);
        return -1;
    }
    w->rows = rows;
    return 0;
}

void penalty_ws_free(dev_pool &mem, penalty_ws *w) {
    mem.put(w->list);
    mem.put(w->count);
    *w = penalty_ws{};
}

int launch_penalty_apply(const penalty_args &a, const penalty_ws &w, hipStream_t s) {
    if (!args_ok(a, w)) return -1;
    hipLaunchKernelGGL(k_penalty_apply, dim3(a.rows), dim3(PN_TH), 0, s, a, w.list, w.count);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

int launch_penalty_restore(const penalty_args &a, const penalty_ws &w, hipStream_t s) {
    if (!args_ok(a, w)) return -1;
    hipLaunchKernelGGL(k_penalty_restore, dim3(a.rows), dim3(PN_TH), 0, s, a, (const uint2 *)w.list, w.count);
    GHIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace ghip
