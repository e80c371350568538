// matvec_rr.hip — the round-pipelined K-split matvec ("rr" form, launch_matvec ks = KS_RR).
//
// Same arithmetic as k_matvec (matvec_impl.h): ggml's AVX2 lane order, one thread per AVX2 lane,
// lane l of row r runs fmaf(d_w*d_a, isum_l, acc) block after block — so results are bit-identical
// to the CPU path (src/hpc.cpp:15-41 calling ggml_vec_dot_q4_0_q8_0 / q8_0_q8_0).
//
// Why another form: at batch 1 a workgroup owns ONE 8-row tile (2048-row matrices have 256 tiles
// for 256 CUs), so its whole K range must be in flight at once and its 64 lane chains are serial
// over K.  The KS = 8 form (k_matvec) gives wave w the contiguous segment w of K and lets wave 0
// carry the chains through segments 1..7 only after ALL loads have landed: the ~450-step carry
// (~1.5 us) sits behind the stream.  Here:
//   * 8 loader waves take block tiles w, w+8, w+16, ... (K interleaved by rounds), so round r's
//     tiles 8r..8r+7 are issued together, early rounds first;
//   * loaders turn round r into exact (d, isum) terms in an LDS slot (two slots, ping-pong);
//   * a 9th wave, the carrier, runs the 64 chains through round r-1 while the loaders convert
//     round r — the chain is consumed as the data lands and ends one round after the last load.
//
// Shape of the code, one generic body (rr_path) in two forms:
//   * a ring that is refilled (D < NR: the down kernels) runs SPLIT: the loader waves and the carrier wave
//     each run their OWN straight-line path, split before the first load: the front (activation loads,
//     the carrier's residual), the image build and all NR rounds.  Both paths pass the same barriers (the
//     front's, the image build's, one in front of the rounds, one per round: none sits under `if (LD)`).
//     A loader's ring loads, its refills and their waits sit on a path that no other path joins, so the
//     compiler's counted waits are exact — vmcnt(2(D-1)+1), vmcnt(2(D-1)) in every round that is followed
//     by a refill, then counting down to 0 over the last D rounds; never a vmcnt(0) drain while refills
//     are in flight (scripts/rr_waits.py prints them, tests/test_rr_waits.py holds them).  With the refill
//     under an `if (loader)` that rejoined the carrier's path every round, the join's merged counters lost
//     two loads per round and the waits fell to (5,4) (3,2) (0) ... : DESIGN.md §5.
//   * a one-shot ring (D = NR: qkv, attn-out, every other instantiation) has no refill to count and keeps
//     the joined form: one path, `if (loader)` per round.  Straight-line paths cost it registers for
//     nothing (the NR 2 / 3 kernels went from 46-62 to 140-168 VGPRs, and those that hold four activation
//     blocks per thread spilled).
#include <type_traits>

#include "matvec_rr.h"

namespace ghip {
namespace {

// E: rounds of the weight ring a loader issues at the front — behind EVERY wave's activation loads
// (one s_barrier orders the issue across the workgroup) and before the image is built; the other
// D - E rounds of the ring go behind the image.  0 = the whole ring behind the image.  Per class,
// chosen by measurement; A/B builds override (scripts/build_variant.sh).
#ifndef GHIP_RR_E_QKV
#define GHIP_RR_E_QKV 0
#endif
#ifndef GHIP_RR_E_OUT
#define GHIP_RR_E_OUT 0
#endif
#ifndef GHIP_RR_E_DOWN
#define GHIP_RR_E_DOWN 2
#endif

// Launch front: the fields the first activation and weight loads are addressed with
// come as leading scalar parameters (14 dwords, the user-SGPR preload's reach on gfx950) and replace
// the struct's copies, so the body below is written against one mv_args.  act2 is the activation's
// second pointer: x_da for PRO_IMG, norm_w otherwise.
template <int WT, int PRO, int EPI, int NR, int R, int DD, int EE>
__global__ void __launch_bounds__(RR_NTH) k_matvec_rr(const void *x, const float *act2, const uint8_t *qs, const uint8_t *sc,
                                                      int64_t n_bt, int64_t nb, int64_t x_col_stride, mv_args a_rest) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    mv_args a = a_rest;
    a.x = x; a.qs = qs; a.sc = sc; a.n_bt = n_bt; a.nb = nb; a.x_col_stride = x_col_stride;
    if (PRO == PRO_IMG) a.x_da = act2;
    else a.norm_w = act2;
    using G = rr_geom<WT>;
    constexpr int BT = G::BT, SB = wfmt<WT>::SCALE_BYTES;
    constexpr bool NSA = true;
    // PRO_IMG: the image's 18 * NR * BT items fit the 2R prefetched per thread (launch_rr_t's R), so the
    // builder's long-K loop (a load and a full wait behind the front's ring rounds) is compiled out
    static_assert(PRO != PRO_IMG || 18 * NR * BT <= 2 * R * RR_NTH, "PRO_IMG: R must cover the whole image");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane >> 3, l = lane & 7;
    const int col = blockIdx.y;
    const int64_t rt = blockIdx.x;
    const lds_map m = make_lds_map<WT, NSA>(1, a.n_bt, a.n_bt, 0);
    const size_t slot0 = (m.total + 15) & ~(size_t)15;
    const bool loader = wave < RR_NL;
    unsigned long long *stp = GHIP_STAMPS && a.dbg_t ? a.dbg_t + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 : nullptr;
    // Stamps (GHIP_STAMPS builds) are taken into registers and stored after the wave's last round: loads and
    // stores share vmcnt and may complete out of order, so one stamp stored while ring loads are pending turns
    // every later wait of the wave into a full drain, and the timeline read back is not the product's.
    unsigned long long ts[16] = {};
    auto stamp = [&](int i) {
        if (GHIP_STAMPS) ts[i] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);

    constexpr int D = DD < NR ? DD : NR;  // ring depth: rounds in flight per loader wave
    constexpr int E = EE < D ? EE : D;    // of them, issued before the image is built
    constexpr bool SPLIT = D < NR;        // the ring is refilled: loaders and carrier on separate paths
    static_assert(E == 0 || SPLIT, "rounds in front of the image: only in the split form");
    const uint32_t q_off = (uint32_t)lane * 16u, s_off = (uint32_t)rr * SB;
    auto slot_s = [&](int r) { return (float *)(smem + slot0 + (size_t)(r & 1) * G::SLOT); };
    auto slot_d = [&](int r) { return (float *)(smem + slot0 + (size_t)(r & 1) * G::SLOT + G::S_BYTES); };
    const int crow = rr;  // the carrier's lane = (row, AVX2 lane) of the loaders' numbering

    // The kernel body.  SPLIT: instantiated once per kind of wave, LD a constant (a loader's path / the
    // carrier's), split before the first load so that no loaded register crosses the split (a copy there would
    // wait for the load).  Joined: once, LD = this wave is a loader.  Every barrier below is outside `if (LD)`,
    // so loaders and carrier pass the same number of them by construction.
    auto rr_path = [&](auto is_loader) __attribute__((always_inline)) {
        const bool LD = is_loader;
        // 0) the front: every wave's activation loads.  The Q8_0 activation image has to be in LDS
        //    before the first round: issued behind the weight stream, the activation loads queue behind
        //    it in the fabric (stamps: image ready at ~4 us of a 9.5 us down); alone they return in ~1 us.
        act_regs<R> ar;
        prefetch_activation<WT, PRO, R, RR_NTH>(a, col, ar);
        // EPI_ADD: the residual of the lanes' rows (the carrier's storing lanes use it) right behind the
        // activation loads, so the epilogue waits for no memory.  Four activation blocks held in registers
        // over the image build (R 4): after the build, when those registers are free again, still
        // microseconds before the last round.  Split: the carrier alone; joined: every wave, because the
        // load in the carrier's branch made the compiler copy the loaders' ring registers at the join,
        // with a full wait behind the ring loads.
        constexpr bool RESID_EARLY = R == 1 || PRO == PRO_IMG;
        float held = 0.0f;
        auto take_resid = [&]() {
            __builtin_amdgcn_sched_barrier(0);  // its address waits for struct fields: after the activation loads
            // uniform base, 32-bit lane offset: the rows left from this tile's first, clamped into the matrix
            const int64_t left = a.rows - 1 - rt * 8;
            const uint32_t ro = (uint32_t)rr < (uint32_t)left ? (uint32_t)rr : (uint32_t)left;
            held = (a.resid + (int64_t)col * a.y_col_stride + rt * 8)[ro];
        };
        if (EPI == EPI_ADD && RESID_EARLY && (!SPLIT || !LD)) take_resid();
        // E > 0: no loader's ring load may precede a slower wave's activation loads on this CU (in each
        // wave's own program order it can, and the activation then queues behind weights: §10).  The
        // barrier waits for no load.
        if (E > 0) __builtin_amdgcn_s_barrier();
        // the ring (loader w, round r -> block tile w + 8r; D rounds in flight per wave)
        uint4 qb[D], sb[D];
        auto issue = [&](int r) {
            const int64_t tile = rt * a.n_bt + wave + RR_NL * r;
            qb[r % D] = ld_nt16(a.qs + tile * 1024 + q_off);
            sb[r % D] = ld_scale<WT>(a.sc + tile * 8 * SB + s_off);
        };
        if (LD) {
#pragma unroll
            for (int r = 0; r < E; ++r) {
                issue(r);
                __builtin_amdgcn_sched_barrier(0);  // round by round: a later round's load in front of this round's scales costs its wait a load
            }
        }
        // 1) the image; its wait is counted: the activation registers only, the E rounds stay in flight
        norm_state ns;
        if (!(MV_ABLATE(a) & 1)) ns = build_activation<WT, PRO, R, NSA, RR_NTH, false>(a, col, smem, m, ar);  // timing ablations only
        if (EPI == EPI_ADD && !RESID_EARLY && (!SPLIT || !LD)) take_resid();
        stamp(10);
        // 2) the rest of the ring, behind the image
        if (LD) {
#pragma unroll
            for (int r = E; r < D; ++r) {
                issue(r);
                if (SPLIT) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the norm's check (PRO_NORM / PRO_EMBED) with the weights already in flight: off the path to
        // the first weight load (measured: +0.35-0.45 us on qkv with the check in front of the issue);
        // the fallback reloads x and w, so only the ring's D rounds stay live beside it
        if (!(MV_ABLATE(a) & 1)) finish_activation<WT, PRO, R, NSA, RR_NTH>(a, col, smem, m, ar, ns);
        stamp(11);
        lds_barrier();
        stamp(1);
        // the carrier's dependent fmaf chain is the critical path: first pick of the SIMD's issue slots
        if (!LD) __builtin_amdgcn_s_setprio(3);

        // 3) rounds: loaders stash round r while the carrier chains round r-1
        float acc = 0.0f;
        auto chain = [&](int r) {
            const float4 *pd = (const float4 *)(slot_d(r) + (size_t)crow * G::SBPD);
            const uint4 *ps = (const uint4 *)(slot_s(r) + (size_t)(crow * 8 + l) * G::SBP);
            acc = carry_ring<false>(ps, pd, G::RUN / 4, acc);  // chunks of 4 blocks: (s, d) f32 pairs
        };
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (LD) {
                float *st = slot_s(r) + (size_t)lane * G::SBP;
                float *sd = slot_d(r) + (size_t)rr * G::SBPD;
                const uint4 q = qb[r % D], scv = sb[r % D];
                if (MV_ABLATE(a) & 8)  // timing only: consume the loads without the dot products
                    acc += __builtin_bit_cast(float, q.x ^ scv.y);
                else
                    rr_stash<WT>(q, scv, smem, m, wave + RR_NL * r, l, st, sd, wave * BT);
                if (r + D < NR) issue(r + D);
                if (r < 8) stamp(2 + r);
                if (r == NR - 1) stamp(15);
            } else if (r > 0 && !(MV_ABLATE(a) & 4)) {
                chain(r - 1);
                if (r == 6) stamp(12);
            }
            lds_barrier();
        }
        if (LD) {
            if ((MV_ABLATE(a) & 8) && acc == 1.2345f) a.y[0] = acc;  // keeps the ablated loads live
            if (GHIP_STAMPS && stp && lane == 0 && wave == 0) {  // slots 0, 1, 2..9, 10, 11: loader wave 0
                stp[0] = ts[0]; stp[1] = ts[1]; stp[10] = ts[10]; stp[11] = ts[11];
#pragma unroll
                for (int r = 0; r < (NR < 8 ? NR : 8); ++r) stp[2 + r] = ts[2 + r];
            }
            if (GHIP_STAMPS && stp && lane == 0 && wave == RR_NL - 1) stp[15] = ts[15];  // the last loader's last round
        } else {
            if (!(MV_ABLATE(a) & 4)) chain(NR - 1);
            stamp(13);
            const float v = fold8(acc);
            unsigned long long best = 0;
            if (l == 0) {
                if (EPI == EPI_ADD) epilogue_held(a, col, rt * 8 + crow, v, held);
                else epilogue<EPI>(a, col, rt * 8 + crow, v, 0.0f, best);
            }
            stamp(14);
            if (GHIP_STAMPS && stp && lane == 0) {  // slots 12..14: the carrier
                stp[12] = ts[12]; stp[13] = ts[13]; stp[14] = ts[14];
            }
        }
    };
    if (!SPLIT) rr_path(loader);
    else if (loader) rr_path(std::true_type{});
    else rr_path(std::false_type{});
}


template <int WT, int PRO, int EPI, int NR>
int launch_rr_t(const mv_args &a, hipStream_t s) {
    constexpr int BT = wfmt<WT>::BT;
    // activation registers per thread.  PRO_IMG: all 18 * NR * BT image items (2R per thread; R 2 for the
    // Gemma-7B down's K 24576), so the builder needs no load of its own behind the front
    constexpr int R = PRO == PRO_IMG                                          ? (18 * NR * BT + 2 * RR_NTH - 1) / (2 * RR_NTH)
                      : (PRO == PRO_F32 || PRO == PRO_NORM) && NR * BT * 8 > 144 ? 4
                                                                                 : 1;
    const lds_map m = make_lds_map<WT, true>(1, a.n_bt, a.n_bt, 0);
    const size_t lds = ((m.total + 15) & ~(size_t)15) + 2 * rr_geom<WT>::SLOT;
    if (lds > 160 * 1024) {
        set_error("matvec(rr): LDS image too large");
        return -1;
    }
    if (PRO == PRO_IMG && a.nb % 4) {
        set_error("matvec(rr): PRO_IMG needs K % 128 == 0");
        return -1;
    }
    // ring depth (rounds in flight per loader wave), measured on the down shape (NR 8), rounds issued
    // after the image: all 8 at once 8.2 us, 6 8.1, 4 7.9, 2 8.2 — four keep the CU's memory queue
    // full without stalling the first round's issue.  (Rounds issued before the image: 8.4 / 8.5 vs
    // 7.95 us; the ring right behind the activation loads: decode 1,449-1,456 vs 1,513-1,517 tok/s —
    // both removed.  Neither ordered the issue across the workgroup's waves, and both ran with the ring's
    // waits inexact; behind every wave's activation loads and one s_barrier, two rounds in front of the
    // image pay on the down: GHIP_RR_E_DOWN)
    constexpr bool deep = (PRO == PRO_IMG || PRO == PRO_F32) && EPI == EPI_ADD && NR >= 8;
    // NR 16 (the Q8_0 down: 16 rounds of 8 tiles) keeps 8 rounds in flight: Q8_0 decode 1,158-1,177 vs
    // 1,209 tok/s at 8 (1,191-1,193 at 6), while the Q4_0 down (NR 8) is best at 4 (1,540-1,544 vs
    // 1,535 at 6, 1,523 at 8) — same box, interleaved; NR 12 (the Gemma-7B down) at 6: the 7B leg
    // 556.7 vs 548.8 tok/s (554 at 8)
    constexpr int DD = !deep ? 64 : NR >= 16 ? 8 : NR >= 12 ? 6 : 4;
    // rounds of the ring at the front, by class: qkv (the normed input), attn-out and down (EPI_ADD).  Not the
    // embedding prologue: its image build loads the embedding row, and those loads would wait for the ring
    constexpr int EE = PRO == PRO_NORM                       ? GHIP_RR_E_QKV
                       : EPI != EPI_ADD                       ? 0
                       : deep                                 ? GHIP_RR_E_DOWN
                                                              : GHIP_RR_E_OUT;
    const void *fn = (const void *)k_matvec_rr<WT, PRO, EPI, NR, R, DD, EE>;
    if (lds > 64 * 1024) GHIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    mv_args la = a;
    const float *act2 = PRO == PRO_IMG ? la.x_da : la.norm_w;
    void *args[] = {(void *)&la.x, (void *)&act2, (void *)&la.qs, (void *)&la.sc, (void *)&la.n_bt, (void *)&la.nb,
                    (void *)&la.x_col_stride, (void *)&la};
    GHIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)a.n_rt, a.ncols), dim3(RR_NTH), args, lds, s));
    GHIP_CHECK(hipGetLastError());
    return 0;
}

template <int WT, int NR>
int rr_pro(int pro, int epi, const mv_args &a, hipStream_t s) {
    if (pro == PRO_Q8 && epi == EPI_STORE) return launch_rr_t<WT, PRO_Q8, EPI_STORE, NR>(a, s);
    if (pro == PRO_NORM && epi == EPI_STORE) return launch_rr_t<WT, PRO_NORM, EPI_STORE, NR>(a, s);
    if (pro == PRO_EMBED && epi == EPI_STORE) return launch_rr_t<WT, PRO_EMBED, EPI_STORE, NR>(a, s);
    if (pro == PRO_F32 && epi == EPI_ADD) return launch_rr_t<WT, PRO_F32, EPI_ADD, NR>(a, s);
    if (pro == PRO_IMG && epi == EPI_ADD) return launch_rr_t<WT, PRO_IMG, EPI_ADD, NR>(a, s);
    if (pro == PRO_F32 && epi == EPI_STORE) return launch_rr_t<WT, PRO_F32, EPI_STORE, NR>(a, s);
    set_error("matvec(rr): (prologue, epilogue) combination not instantiated");
    return -1;
}

}  // namespace

// n_bt block tiles per row = 8 loaders x NR rounds; NR in {1, 2, 3, 8, 12, 16}
bool matvec_rr_supported(int wtype, int64_t n_bt) {
    if (wtype != T_Q4_0 && wtype != T_Q8_0) return false;
    if (n_bt % RR_NL) return false;
    const int64_t nr = n_bt / RR_NL;
    return nr == 1 || nr == 2 || nr == 3 || nr == 8 || nr == 12 || nr == 16;
}

int matvec_dispatch_rr(int wtype, int pro, int epi, const mv_args &a, hipStream_t s) {
    if (!matvec_rr_supported(wtype, a.n_bt)) {
        set_error("matvec(rr): block tiles per row must be 8 x {1,2,3,8,12,16}");
        return -1;
    }
    const int nr = (int)(a.n_bt / RR_NL);
#define RR_CASE(N)                                                         \
    case N:                                                                \
        return wtype == T_Q4_0 ? rr_pro<T_Q4_0, N>(pro, epi, a, s) : rr_pro<T_Q8_0, N>(pro, epi, a, s);
    switch (nr) {
        RR_CASE(1)
        RR_CASE(2)
        RR_CASE(3)
        RR_CASE(8)
        RR_CASE(12)
        RR_CASE(16)
    }
#undef RR_CASE
    return -1;
}

}  // namespace ghip
