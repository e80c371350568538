// engine_diag.cpp — what measures, tunes and inspects the device-resident engine: per-kernel
// timing, the launch-plan tuner, plan / option setters, phase stamps (the entry points that need a
// -DGHIP_STAMPS=1 build of this file), per-layer taps, the per-op test hooks and the HBM probes.
#include "engine_impl.h"

// ---- hipEvent timing of one hot kernel on the engine stream (bench.py roofline leg) -----------
extern "C" double gemma_engine_time(gemma_engine *e, int which, int iters, double *algo_bytes) {
    set_error("");
    (void)hipSetDevice(e->device);
    const gemma_hip_config &c = e->cfg;
    const int wt = c.wtype;
    // launches rotate over the layers' matrices, as in a decode step: each launch reads its weights
    // cold (18 x the FFN matrices exceed the 256 MB Infinity Cache)
    int layer = 0;
    mv_args a;
    int ks = 1, pro = PRO_F32, epi = EPI_STORE, grid = 1;
    double bytes = 0;
    auto setup = [&](layer_dev &L) {
    switch (which) {
        case 0:
            set_mat(a, L.gate);
            a.qs2 = L.up.qs; a.sc2 = L.up.sc;
            a.x = e->sa; a.norm_w = L.ffn_norm; a.eps = c.eps; a.y = e->h; a.gelu_tab = e->gelu_tab;
            pro = PRO_NORM; epi = EPI_GELU_MUL; ks = e->plan[MC_GU].ks;  // 2 = gate and up on separate waves
            grid = mv_grid(e, MC_GU, L.gate.n_rt);
            bytes = (double)L.gate.algo_bytes() + L.up.algo_bytes() + c.n_embd * 4.0 * 2 + c.n_ff * 4.0;
            break;
        case 1:
            set_mat(a, L.down);
            a.x = e->h; a.y = e->x; a.resid = e->sa; ks = pick_ks(wt, L.down.n_bt, e->plan[MC_DOWN].ks); epi = EPI_ADD;
            if (e->h_act && e->plan[MC_DOWN].img) { a.x = e->h_act; a.x_da = e->h_da; pro = PRO_IMG; }
            grid = mv_grid(e, MC_DOWN, L.down.n_rt);
            bytes = (double)L.down.algo_bytes() + c.n_ff * (e->h_act ? 36.0 / 32 : 4.0) + c.n_embd * 8.0;
            break;
        case 2:
            set_mat(a, L.qkv);
            a.x = e->x; a.norm_w = L.attn_norm; a.eps = c.eps; a.y = e->qkv; ks = pick_ks(wt, L.qkv.n_bt, e->plan[MC_QKV].ks); pro = PRO_NORM;
            grid = mv_grid(e, MC_QKV, L.qkv.n_rt);
            bytes = (double)L.qkv.algo_bytes() + c.n_embd * 8.0 + e->qkv_rows * 4.0;
            break;
        case 3:
            set_mat(a, L.o);
            a.x = e->attn; a.y = e->sa; a.resid = e->x; ks = pick_ks(wt, L.o.n_bt, e->plan[MC_O].ks); epi = EPI_ADD;
            if (e->att_act && att_img_ok(e) && e->plan[MC_O].img) { a.x = e->att_act; a.x_da = e->att_da; pro = PRO_IMG; }
            grid = mv_grid(e, MC_O, L.o.n_rt);
            bytes = (double)L.o.algo_bytes() + e->qw * (pro == PRO_IMG ? 36.0 / 32 : 4.0) + c.n_embd * 8.0;
            break;
        case 4:
            set_mat(a, e->embd);
            a.x = e->x; a.norm_w = e->out_norm; a.eps = c.eps; a.y = e->logits; a.argmax_key = e->key;
            pro = PRO_NORM; epi = EPI_ARGMAX;
            grid = mv_grid(e, MC_LOGITS, e->embd.n_rt);
            bytes = (double)e->embd.algo_bytes() + c.n_embd * 8.0 + c.n_vocab * 4.0;
            break;
        default:
            break;
    }
    };
    if (e->kq) {
        set_error("gemma_engine_time: K-quant layer engines time their matvecs with gemma_kq_time");
        return -1.0;
    }
    if (which == 4 && e->out_type == T_Q6_K) {
        set_error("gemma_engine_time: the logits kernel of a Q6_K output is the K-quant matvec (gemma_kq_time)");
        return -1.0;
    }
    if (which < 0 || which > 5) {
        set_error("gemma_engine_time: bad kernel id");
        return -1.0;
    }
    setup(e->layers[0]);
    const bool hot = e->time_hot != 0;
    a.ablate = e->ablate;
    auto run = [&]() -> int {
        if (which == 5) {
            if (ensure_graph(e)) return -1;
            GHIP_CHECK(hipGraphLaunch(e->graph_exec, e->stream));
            return 0;
        }
        if (which < 4) {
            setup(e->layers[layer]);
            if (!hot) layer = (layer + 1) % c.n_layer;  // hot: the same matrix (Infinity-Cache resident)
        }
        return launch_matvec(wt, ks, pro, epi, a, grid, e->stream);
    };
    if (which == 5) {
        // whole step replays advance the position: keep within the context
        if (e->seq.host_pos + 2 * iters + 4 >= c.n_ctx) {
            set_error("gemma_engine_time: context too small for step timing");
            return -1.0;
        }
    }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    float ms = 0;
    auto timed = [&]() -> int {
        GHIP_CHECK(hipEventCreate(&t0));
        GHIP_CHECK(hipEventCreate(&t1));
        for (int i = 0; i < 3; ++i)
            if (run()) return -1;
        GHIP_CHECK(hipEventRecord(t0, e->stream));
        for (int i = 0; i < iters; ++i)
            if (run()) return -1;
        GHIP_CHECK(hipEventRecord(t1, e->stream));
        GHIP_CHECK(hipEventSynchronize(t1));
        GHIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
        return 0;
    };
    const int tr = timed();
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (tr) return -1.0;
    if (which == 5) e->seq.host_pos += iters + 3;
    if (algo_bytes) *algo_bytes = bytes;
    return (double)ms * 1000.0 / iters;
}

// ---- launch-plan tuning -----------------------------------------------------------------------
// Coordinate descent over the matrix classes: for each class every feasible (K split, row-tile
// groups per workgroup) is timed as whole decode steps (hipGraph replays on a fresh context), the
// other classes held at their current best.  Whole steps keep the cache state of real decoding
// (a matrix timed alone would be served from the 256 MB Infinity Cache).  Every candidate computes
// the same bits (the K split keeps the block order), so tuning changes speed only.  The decode
// state is clobbered: call gemma_engine_begin afterwards.  In a TP job every rank runs the same
// candidate sequence (same collectives per step); ranks may settle on different plans.
extern "C" int gemma_engine_tune(gemma_engine *e, int iters) {
    set_error("");
    if (e->kq) return 0;  // K-quant layers: no launch plan to measure
    (void)hipSetDevice(e->device);
    const gemma_hip_config &c = e->cfg;
    const int wt = c.wtype;
    const int32_t prompt[4] = {2, 2, 2, 2};
    iters = std::max(2, std::min(iters, c.n_ctx - 12));
    if (iters < 2 || c.n_ctx < 16) {
        set_error("gemma_engine_tune: context too small");
        return -1;
    }
    hipEvent_t t0, t1;
    GHIP_CHECK(hipEventCreate(&t0));
    GHIP_CHECK(hipEventCreate(&t1));
    auto trial = [&]() -> double {
        drop_graph(e);
        if (gemma_engine_begin(e, prompt, 4)) return -1.0;
        if (gemma_engine_step(e, 1, nullptr, 1)) return -1.0;  // eager step + capture
        for (int i = 0; i < 2; ++i)
            if (hipGraphLaunch(e->graph_exec, e->stream) != hipSuccess) return -1.0;
        // the minimum of three timed runs: one run's box noise (±1 %) exceeded the differences
        // between neighbouring plans, so single samples picked plans by luck (round 5: the bench's
        // logits plan varied run to run between 1, 2 and 8 row tiles per workgroup, ±2 µs)
        double tmin = 1e30;
        for (int rep = 0; rep < 3; ++rep) {
            if (hipEventRecord(t0, e->stream) != hipSuccess) return -1.0;
            for (int i = 0; i < iters; ++i)
                if (hipGraphLaunch(e->graph_exec, e->stream) != hipSuccess) return -1.0;
            if (hipEventRecord(t1, e->stream) != hipSuccess || hipEventSynchronize(t1) != hipSuccess) return -1.0;
            float ms = 0;
            (void)hipEventElapsedTime(&ms, t0, t1);
            tmin = std::min(tmin, (double)ms * 1000.0 / iters);
        }
        return tmin;
    };
    const layer_dev &L0 = e->layers[0];
    const int64_t nbt[MC_N] = {L0.qkv.n_bt, L0.o.n_bt, L0.gate.n_bt, L0.down.n_bt, e->embd.n_bt};
    int rc = 0;
    double best = trial();
    if (best < 0) rc = -1;
    const int order[MC_N] = {MC_DOWN, MC_GU, MC_QKV, MC_O, MC_LOGITS};
    for (int oi = 0; oi < MC_N && rc == 0; ++oi) {
        const int cls = order[oi];
        if (cls == MC_LOGITS && e->out_type == T_Q6_K) continue;  // the K-quant matvec has no plan
        std::vector<launch_plan> cands;
        const bool splits = cls == MC_QKV || cls == MC_O || cls == MC_DOWN || cls == MC_GU;
        for (int ks = 1; ks <= (cls == MC_GU ? 2 : splits ? 8 : 1); ks *= 2) {
            if (pick_ks(wt, nbt[cls], ks) != ks) continue;  // not a divisor, or the LDS image overflows
            const int rmax = cls == MC_LOGITS ? 16 : ks == 1 ? 2 : 4;
            for (int rpw = 1; rpw <= rmax; rpw *= 2) cands.push_back({ks, rpw, e->plan[cls].img});
        }
        // the round-pipelined form (one workgroup per row tile)
        if (splits && cls != MC_GU && pick_ks(wt, nbt[cls], KS_RR) == KS_RR) cands.push_back({KS_RR, 1, e->plan[cls].img});
        const launch_plan keep = e->plan[cls];
        launch_plan win = keep;
        // whole steps for every class.  (Timing the logits launch alone picked 1 row tile per
        // workgroup, whose back-to-back launches overlap their tails; inside the step, where k_advance
        // waits for it, 8 measured 52.3-52.7 vs 53.2-54.4 µs — round 5, driver-style bench lines.)
        auto measure = [&]() -> double { return trial(); };
        double best_cls;
        {  // the incumbent re-measured beside its challengers (not a sample from an earlier class)
            const double t = measure();
            if (t < 0) {
                rc = -1;
                break;
            }
            best_cls = t;
        }
        for (const launch_plan &p : cands) {
            if (p.ks == keep.ks && p.rpw == keep.rpw && p.img == keep.img) continue;
            e->plan[cls] = p;
            const double t = measure();
            if (t < 0) {
                rc = -1;
                break;
            }
            if (t < best_cls * 0.998) {  // a challenger must beat the incumbent past the noise floor
                best_cls = t;
                win = p;
            }
        }
        e->plan[cls] = win;
        if (cls != MC_LOGITS) best = best_cls;
        // on / off switches: the incumbent re-measured beside the challenger and the same 0.2 %
        // hysteresis as the plans (a bare t < best flipped on noise).  Every condition is
        // structural, never a measured outcome, so every rank of a TP job runs the same trials.
        auto toggle = [&](auto flip) {
            if (rc) return;
            const double inc = trial();
            flip();
            const double t = inc < 0 ? -1.0 : trial();
            if (t < 0) rc = -1;
            if (t >= 0 && t < inc * 0.998) best = t;
            else flip();
        };
        if (cls == MC_O && e->ag.nwg && e->cfg.n_ctx <= 2048 && e->cfg.head_dim <= 256)
            toggle([&] { e->att_mode ^= 1; });  // attention form: one workgroup per head vs the split
        // the producer-written activation image, at the winning launch shape
        if ((cls == MC_O && e->att_act) || (cls == MC_DOWN && e->h_act)) toggle([&] { e->plan[cls].img ^= 1; });
        // attention + attn-out in one launch (takes effect with the image and the rr attn-out form)
        if (cls == MC_O && e->ao_cnt && e->n_virtual == 1) toggle([&] { e->att_o ^= 1; });
    }
    drop_graph(e);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    e->seq.host_pos = 0;
    return rc;
}

// the current plan, 3 ints per class (qkv, o, gate/up, down, logits): K split, row-tile groups per
// workgroup, activation image (o, down); returns the number of ints written
extern "C" int gemma_engine_plan(gemma_engine *e, int *out, int cap) {
    int n = 0;
    for (int cls = 0; cls < MC_N && n + 3 <= cap; ++cls) {
        out[n++] = e->plan[cls].ks;
        out[n++] = e->plan[cls].rpw;
        out[n++] = e->plan[cls].img;
    }
    if (n < cap) out[n++] = e->att_mode;  // attention form: 0 per head, 1 split
    return n;
}

// kernel launches per decode token: the kernel nodes of the captured decode graph (captured on
// first use if needed); -1 on error
extern "C" int gemma_engine_graph_kernels(gemma_engine *e) {
    set_error("");
    (void)hipSetDevice(e->device);
    if (!e->graph) {
        set_error("gemma_engine_graph_kernels: no decode graph yet (run a gemma_engine_step with use_graph first)");
        return -1;
    }
    size_t n = 0;
    GHIP_CHECK(hipGraphGetNodes(e->graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    GHIP_CHECK(hipGraphGetNodes(e->graph, nodes.data(), &n));
    int k = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        GHIP_CHECK(hipGraphNodeGetType(nodes[i], &t));
        k += t == hipGraphNodeTypeKernel;
    }
    return k;
}

// the persistent token launch on/off (-1 = keep); returns 1 when it runs this engine's decode
// steps, 0 when not (hpc_last_error says why if it was asked for)
extern "C" int gemma_engine_set_persist(gemma_engine *e, int on) {
    set_error("");
    (void)hipSetDevice(e->device);
    if (on > 0 && e->penalising) {
        set_error("gemma_engine_set_persist: penalties are on (gemma_engine_set_penalties): they run with the per-layer launches");
        return -1;
    }
    if (on >= 0 && on != e->persist) {
        e->persist = on;
        drop_graph(e);
    }
    if (tok_prepare(e)) return -1;
    if (e->persist && !e->persist_why.empty()) set_error("persistent token launch: " + e->persist_why);
    return persist_on(e) ? 1 : 0;
}

// tests: the persistent launch's per-wait bound in 100 MHz ticks (0 = the default 20 ms); a tiny
// bound forces hand-off timeouts so that their reporting can be checked
extern "C" int gemma_engine_set_persist_timeout(gemma_engine *e, unsigned ticks) {
    set_error("");
    (void)hipSetDevice(e->device);
    e->persist_timeout = ticks ? ticks : 2000000u;
    drop_graph(e);
    return tok_prepare(e);
}

// the persistent launch's sticky hand-off timeout words [flag, site, layer] (0 = none seen);
// reset = 1 clears them
extern "C" int gemma_engine_persist_err(gemma_engine *e, int *out3, int reset) {
    (void)hipSetDevice(e->device);
    int w[3] = {0, 0, 0};
    if (e->tok_err) GHIP_CHECK(hipMemcpy(w, e->tok_err, 12, hipMemcpyDeviceToHost));
    if (out3) memcpy(out3, w, 12);
    if (reset && e->tok_err) GHIP_CHECK(hipMemset(e->tok_err, 0, 64));
    return w[0];
}

// Engine options (tests, A/B): the measured variants that stay selectable, set through the API so a
// stray environment variable on a box can never change the benched kernels.  Returns 0, or -1 for an
// unknown name.  The decode graph is dropped (re-captured at the next step).
extern "C" int gemma_engine_set_option(gemma_engine *e, const char *name, int value) {
    set_error("");
    const std::string n = name ? name : "";
    int *f = n == "kq_fuse" ? &e->kq_fuse : n == "kq_dual" ? &e->kq_dual : n == "kq_pair" ? &e->kq_pair : n == "kq_skinny" ? &e->kq_skinny
           : n == "kq_abl" ? &e->kq_abl : n == "att_mx" ? &e->att_mx : n == "att_win" ? &e->att_win : n == "time_hot" ? &e->time_hot
           : n == "ablate" ? &e->ablate : n == "ks_small" ? &e->ks_small : n == "ks_down" ? &e->ks_down : nullptr;
    if (n == "att_dsplit") {
        if (value < 1 || value > 8 || (value & (value - 1)) || e->cfg.head_dim % (32 * value)) {
            set_error("gemma_engine_set_option: att_dsplit must be 1, 2, 4 or 8 and divide head_dim / 32");
            return -1;
        }
        f = &e->att_dsplit;
    }
    if (n == "grid_big") {
        if (value < 1 || value > e->grid_big_cap) {
            set_error("gemma_engine_set_option: grid_big out of range (1 .. the argmax key buffer)");
            return -1;
        }
        f = &e->grid_big;
    }
    if (n == "bt_mfma_min") {
        if (value <= GEMM_SKINNY_MAX_T || value > GEMMA_BATCH_WIDE_MAX_SLOTS + 1) {
            set_error("gemma_engine_set_option: bt_mfma_min must be in [9, 65] (65: never the MFMA form)");
            return -1;
        }
        e->bt_mfma_min = value;  // read at the next batch_step; no captured graph holds a batch pass
        return 0;
    }
    if (!f) {
        set_error("gemma_engine_set_option: unknown option '" + n + "'");
        return -1;
    }
    // the product kernels do not read the flag: a timing taken without the ablation must not pass
    // for one taken with it
    if (!GHIP_ABLATE && n == "ablate" && value != 0) {
        set_error("gemma_engine_set_option: ablate: library built without -DGHIP_ABLATE=1 (scripts/build_variant.sh)");
        return -1;
    }
    *f = value;
    drop_graph(e);
    return 0;
}

// On-device sampling on / off and its parameters (include/gemma_hpc.h).  The parameters live in a
// device struct the sampler's kernels read, and their launch geometry depends on n_vocab only: a new
// seed, temperature, top_k or top_p is a stream-ordered copy and the captured graph is kept; only
// turning sampling on or off, or moving between the truncated sampler's three launches and the
// whole-vocabulary sampler's six (top_k == GEMMA_TOP_K_ALL), changes the node set and drops the graph.
extern "C" int gemma_engine_set_sampler(gemma_engine *e, const gemma_sampler *sp) {
    set_error("");
    if (sp) {
        const std::string why = sampler_invalid(*sp, e->cfg.n_vocab);
        if (!why.empty()) {
            set_error("gemma_engine_set_sampler: " + why);
            return -1;
        }
    }
    const bool on = sp && sp->temperature > 0.0f;
    if (on && (row_split(e) || e->tp_n_keys)) {
        set_error("gemma_engine_set_sampler: row-split engines hold a vocabulary shard per rank; sampling needs the whole row "
                  "(single-GPU engines only)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (on) {
        if (!e->smp_dev) {
            // made once and kept for the engine's lifetime (the captured graph holds both): a workspace
            // per row of a verify pass or a narrow batch pass, the decode step uses the first
            if (sample_ws_alloc(e->mem, &e->smp_ws, e->cfg.n_vocab, e->stream, GEMM_SKINNY_MAX_T)) return -1;
            if (e->mem.get(&e->smp_dev, sizeof(sampler_params))) {
                sample_ws_free(e->mem, &e->smp_ws);
                return -1;
            }
        }
        // the copy's source must outlive the call: wait for an earlier copy before rewriting it
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        e->smp_host = sampler_params{};
        e->smp_host.temperature = sp->temperature; e->smp_host.top_k = sp->top_k; e->smp_host.top_p = sp->top_p;
        e->smp_host.seed = sp->seed;
        GHIP_CHECK(hipMemcpyAsync(e->smp_dev, &e->smp_host, sizeof(sampler_params), hipMemcpyHostToDevice, e->stream));
    }
    const bool was_full = engine_samples_full(e);
    e->smp = sp ? *sp : gemma_sampler{0.0f, 0, 1.0f, 0};
    if (on != e->sampling || (on && sampler_full(e->smp) != was_full)) {
        e->sampling = on;
        drop_graph(e);
    }
    e->bt.dirty = true;  // the rows of an open batch's slots that follow the engine carry these parameters
    return 0;
}

extern "C" int gemma_engine_sampler(const gemma_engine *e, gemma_sampler *out) {
    if (out) *out = e->smp;
    return e->sampling ? 1 : 0;
}

// Penalties on / off and their values (include/gemma_hpc.h).  The values live in a device struct the two
// kernels of penalty.hip read, and their geometry is the row count alone: new values or a new last_n are
// a stream-ordered copy and the captured graph is kept; on / off changes the node set and drops it.
extern "C" int gemma_engine_set_penalties(gemma_engine *e, const gemma_penalties *p) {
    set_error("");
    const std::string fn = "gemma_engine_set_penalties";
    if (p) {
        const std::string why = penalties_invalid(*p);
        if (!why.empty()) {
            set_error(fn + ": " + why);
            return -1;
        }
    }
    const bool on = p && !penalties_off(*p);
    if (on && (row_split(e) || e->tp_n_keys)) {
        set_error(fn + ": row-split engines hold a vocabulary shard per rank; a penalised pick needs the whole row "
                  "(single-GPU engines only)");
        return -1;
    }
    if (on && e->persist) {
        set_error(fn + ": the persistent token launch is on (gemma_engine_set_persist): penalties run with the per-layer launches");
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (on) {
        if (!e->pen_dev) {  // made once and kept for the engine's lifetime (the captured graph holds both)
            if (penalty_ws_alloc(e->mem, &e->pen_ws, e->stream, GEMM_SKINNY_MAX_T)) return -1;
            if (e->mem.get(&e->pen_dev, sizeof(penalty_params))) {
                penalty_ws_free(e->mem, &e->pen_ws);
                return -1;
            }
        }
        // the copy's source must outlive the call: wait for an earlier copy before rewriting it
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        e->pen_host.repeat = p->repeat; e->pen_host.presence = p->presence; e->pen_host.frequency = p->frequency;
        e->pen_host.last_n = p->last_n;
        GHIP_CHECK(hipMemcpyAsync(e->pen_dev, &e->pen_host, sizeof(penalty_params), hipMemcpyHostToDevice, e->stream));
    }
    e->pen = p ? *p : gemma_penalties{1.0f, 0.0f, 0.0f, 64};
    if (on != e->penalising) {
        e->penalising = on;
        drop_graph(e);
    }
    return batch_penalty_ws(e);  // an open batch with wider passes than the engine's 8 rows: its own lists
}

extern "C" int gemma_engine_penalties(const gemma_engine *e, gemma_penalties *out) {
    if (out) *out = e->pen;
    return e->penalising ? 1 : 0;
}

// Test hook: k_penalty_apply and k_penalty_restore on `rows` host rows, each with a history and a position
// of its own through a row table (as a batch pass reads them), up to 64 rows a launch; the rows are
// copied out after each kernel
extern "C" int gemma_test_penalize(const float *logits, int rows, int n_vocab, const int32_t *hist, int hist_ld,
                                   const int32_t *positions, const gemma_penalties *p, float *penalised, float *restored,
                                   int32_t *n_saved) {
    set_error("");
    const std::string fn = "gemma_test_penalize";
    if (!logits || !hist || !positions || !penalised || !restored || !n_saved || rows < 1 || n_vocab < 1 || hist_ld < 1) {
        set_error(fn + ": logits, hist, positions, the three outputs, rows >= 1, n_vocab >= 1 and hist_ld >= 1 are required");
        return -1;
    }
    std::string why = p ? penalties_invalid(*p) : "";
    for (int r = 0; why.empty() && r < rows; ++r)
        if (positions[r] < 0 || positions[r] >= hist_ld) why = "positions must be in [0, hist_ld)";
    if (!why.empty()) {
        set_error(fn + ": " + why);
        return -1;
    }
    dev_pool tmp;
    penalty_ws ws;
    penalty_params hp, *dp = nullptr;  // off unless a setting is given
    if (p) { hp.repeat = p->repeat; hp.presence = p->presence; hp.frequency = p->frequency; hp.last_n = p->last_n; }
    const int chunk = std::min(rows, (int)PICK_MAX_ROWS);
    const size_t row_b = (size_t)n_vocab * 4;
    float *dl = nullptr;
    int *dh = nullptr, *dpos = nullptr;
    slot_row *dtab = nullptr;
    if (penalty_ws_alloc(tmp, &ws, nullptr, chunk)) return -1;
    if (tmp.get(&dp, sizeof(hp)) || tmp.get(&dl, row_b * rows) || tmp.get(&dh, (size_t)rows * hist_ld * 4) ||
        tmp.get(&dpos, (size_t)rows * 4) || tmp.get(&dtab, (size_t)rows * sizeof(slot_row)))
        return -1;
    std::vector<slot_row> htab(rows);
    for (int r = 0; r < rows; ++r) {
        htab[r].hist = dh + (size_t)r * hist_ld;
        htab[r].pos = dpos + r;
    }
    GHIP_CHECK(hipMemcpy(dp, &hp, sizeof(hp), hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dl, logits, row_b * rows, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dh, hist, (size_t)rows * hist_ld * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dpos, positions, (size_t)rows * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dtab, htab.data(), (size_t)rows * sizeof(slot_row), hipMemcpyHostToDevice));
    GHIP_CHECK(hipDeviceSynchronize());  // (the workspace's counts were zeroed on the null stream)
    for (int r = 0; r < rows; r += chunk) {
        const int T = std::min(chunk, rows - r);
        penalty_args a;
        a.lg = dl + (size_t)r * n_vocab; a.ld = n_vocab; a.n_vocab = n_vocab; a.rows = T; a.prm = dp; a.tab = dtab + r;
        a.hist_cap = hist_ld;
        if (launch_penalty_apply(a, ws, nullptr)) return -1;
        GHIP_CHECK(hipDeviceSynchronize());
        GHIP_CHECK(hipMemcpy(penalised + (size_t)r * n_vocab, a.lg, row_b * T, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(n_saved + r, ws.count, (size_t)T * 4, hipMemcpyDeviceToHost));
        if (launch_penalty_restore(a, ws, nullptr)) return -1;
        GHIP_CHECK(hipDeviceSynchronize());
        GHIP_CHECK(hipMemcpy(restored + (size_t)r * n_vocab, a.lg, row_b * T, hipMemcpyDeviceToHost));
    }
    return 0;
}

// Per-token log-probabilities on / off (include/gemma_hpc.h).  On adds k_lse_parts and k_lse_finish
// behind every pick, so the decode graph's node set changes and it is dropped, as for the sampler.
// The engine's 8 rows of partials are made once and kept (the captured graph holds them).
extern "C" int gemma_engine_set_logprobs(gemma_engine *e, int on) {
    set_error("");
    if (on < 0) return e->logprobs ? 1 : 0;
    if (on && (row_split(e) || e->tp_n_keys)) {
        set_error("gemma_engine_set_logprobs: row-split engines hold a vocabulary shard per rank; a log-probability needs the "
                  "whole row (single-GPU engines only)");
        return -1;
    }
    if (on && e->cfg.n_vocab > (int64_t)LSE_MAX_G * LSE_CHUNK) {
        set_error("gemma_engine_set_logprobs: n_vocab above " + std::to_string((int64_t)LSE_MAX_G * LSE_CHUNK));
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (on && !e->lp_parts.parts &&
        e->mem.get(&e->lp_parts.parts, (size_t)GEMM_SKINNY_MAX_T * lse_grid(e->cfg.n_vocab) * sizeof(lse_part)))
        return -1;
    if (!on && e->top_lp && gemma_engine_set_top_logprobs(e, 0) < 0) return -1;  // the alternatives need them
    if ((on != 0) != e->logprobs) {
        e->logprobs = on != 0;
        drop_graph(e);
    }
    return e->logprobs ? 1 : 0;
}

// The n most likely tokens of every scored position (include/gemma_hpc.h), 0 = off.  On adds k_topn_parts
// and k_topn_finish behind the log-probability pair; n is a kernel argument, so any change drops the
// decode graph.  Made when first turned on and kept, sized for GEMMA_TOP_LOGPROBS_MAX (the captured graph
// holds them): the engine's 8 rows of candidates and its own sequence's alternatives.  A batch's slots
// and a wide batch's candidates are made at batch_open by the setting then, so it stays while one is open.
extern "C" int gemma_engine_set_top_logprobs(gemma_engine *e, int n) {
    set_error("");
    const std::string fn = "gemma_engine_set_top_logprobs";
    if (n < 0) return e->top_lp;
    if (n > GEMMA_TOP_LOGPROBS_MAX) {
        set_error(fn + ": n = " + std::to_string(n) + " outside [0, " + std::to_string(GEMMA_TOP_LOGPROBS_MAX) + "]");
        return -1;
    }
    if (n == e->top_lp) return n;
    if (n && row_split(e)) {
        set_error(fn + ": row-split engines hold a vocabulary shard per rank (single-GPU engines only)");
        return -1;
    }
    if (n && !e->logprobs) {
        set_error(fn + ": the alternatives come with the log-probabilities: turn those on first (gemma_engine_set_logprobs)");
        return -1;
    }
    if (e->bt.open) {
        set_error(fn + ": a batch is open: its slots were made for the setting it was opened with (gemma_engine_batch_close)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (n && !e->lp_parts.top &&
        e->mem.get(&e->lp_parts.top, (size_t)GEMM_SKINNY_MAX_T * topn_grid(e->cfg.n_vocab) * GEMMA_TOP_LOGPROBS_MAX * 8))
        return -1;
    if (n && !e->seq.alt_tok) {
        if (seq_alt_alloc(e, e->mem, e->seq)) return -1;
        GHIP_CHECK(hipStreamSynchronize(e->stream));
    }
    e->top_lp = n;
    drop_graph(e);
    return n;
}

// Test hook: the alternatives of `rows` host rows through the four kernels (the log-probability pair and
// the top-n pair), the rows as one sequence: row r predicts sequence index r + 1
extern "C" int gemma_test_top_logprobs(const float *logits, int rows, int n_vocab, int n, int32_t *tokens, double *lps) {
    set_error("");
    if (!logits || !tokens || !lps || rows < 1 || rows > 65535 || n_vocab < 1 || n_vocab > LSE_MAX_G * LSE_CHUNK || n < 1 ||
        n > GEMMA_TOP_LOGPROBS_MAX) {
        set_error("gemma_test_top_logprobs: logits, tokens, lps, rows in [1, 65535], n_vocab in [1, " +
                  std::to_string(LSE_MAX_G * LSE_CHUNK) + "] and n in [1, " + std::to_string(GEMMA_TOP_LOGPROBS_MAX) + "] are required");
        return -1;
    }
    dev_pool tmp;
    float *dl = nullptr;
    int *dpos = nullptr;
    int32_t *dtok = nullptr;
    double *dlp = nullptr;
    lse_part *dp = nullptr;
    unsigned long long *dt = nullptr;
    const size_t row_b = (size_t)n_vocab * 4, alt = (size_t)(rows + 1) * GEMMA_TOP_LOGPROBS_MAX;
    if (tmp.get(&dl, row_b * rows) || tmp.get(&dpos, 4) || tmp.get(&dtok, alt * 4) || tmp.get(&dlp, alt * 8) ||
        tmp.get(&dp, (size_t)rows * lse_grid(n_vocab) * sizeof(lse_part)) || tmp.get(&dt, (size_t)rows * topn_grid(n_vocab) * n * 8))
        return -1;
    GHIP_CHECK(hipMemcpy(dl, logits, row_b * rows, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dpos, &rows, 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemset(dtok, 0xFF, alt * 4));
    GHIP_CHECK(hipMemset(dlp, 0xFF, alt * 8));
    topn_finish_args a;
    a.l.lg = dl; a.l.ld = n_vocab; a.l.n = n_vocab; a.l.R = rows; a.l.G = lse_grid(n_vocab); a.l.n_ctx = rows;
    a.l.parts = dp; a.l.pos = dpos; a.l.alt_tok = dtok; a.l.alt_lp = dlp;
    a.tparts = dt; a.Gt = topn_grid(n_vocab); a.top = n;
    if (launch_lse_parts(dl, n_vocab, rows, n_vocab, dp, nullptr) || launch_topn_parts(dl, n_vocab, rows, n_vocab, n, dt, nullptr) ||
        launch_topn_finish(a, nullptr))
        return -1;
    GHIP_CHECK(hipDeviceSynchronize());
    const size_t W = GEMMA_TOP_LOGPROBS_MAX;
    GHIP_CHECK(hipMemcpy2D(tokens, (size_t)n * 4, dtok + W, W * 4, (size_t)n * 4, (size_t)rows, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy2D(lps, (size_t)n * 8, dlp + W, W * 8, (size_t)n * 8, (size_t)rows, hipMemcpyDeviceToHost));
    return 0;
}

// Test hook: logprob(rows[r], tokens[r]) through the two kernels, the rows as one sequence: row r
// predicts sequence index r + 1, whose token is tokens[r]
extern "C" int gemma_test_logprob(const float *logits, int rows, int n_vocab, const int32_t *tokens, double *out) {
    set_error("");
    if (!logits || !tokens || !out || rows < 1 || rows > 65535 || n_vocab < 1 || n_vocab > LSE_MAX_G * LSE_CHUNK) {
        set_error("gemma_test_logprob: logits, tokens, out, rows in [1, 65535] and n_vocab in [1, " +
                  std::to_string(LSE_MAX_G * LSE_CHUNK) + "] are required");
        return -1;
    }
    for (int r = 0; r < rows; ++r)
        if (tokens[r] < 0 || tokens[r] >= n_vocab) {
            set_error("gemma_test_logprob: token id " + std::to_string(tokens[r]) + " out of range [0, n_vocab)");
            return -1;
        }
    dev_pool tmp;
    float *dl = nullptr;
    int *dh = nullptr, *dpos = nullptr;
    double *dlp = nullptr;
    lse_part *dp = nullptr;
    const size_t row_b = (size_t)n_vocab * 4;
    if (tmp.get(&dl, row_b * rows) || tmp.get(&dh, (size_t)(rows + 1) * 4) || tmp.get(&dpos, 4) ||
        tmp.get(&dlp, (size_t)(rows + 1) * 8) || tmp.get(&dp, (size_t)rows * lse_grid(n_vocab) * sizeof(lse_part)))
        return -1;
    GHIP_CHECK(hipMemcpy(dl, logits, row_b * rows, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemset(dh, 0, 4));
    GHIP_CHECK(hipMemcpy(dh + 1, tokens, (size_t)rows * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dpos, &rows, 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemset(dlp, 0xFF, (size_t)(rows + 1) * 8));
    lse_finish_args a;
    a.lg = dl; a.ld = n_vocab; a.n = n_vocab; a.R = rows; a.G = lse_grid(n_vocab); a.n_ctx = rows;
    a.parts = dp; a.pos = dpos; a.hist = dh; a.lp = dlp;
    if (launch_lse_parts(dl, n_vocab, rows, n_vocab, dp, nullptr) || launch_lse_finish(a, nullptr)) return -1;
    GHIP_CHECK(hipDeviceSynchronize());
    GHIP_CHECK(hipMemcpy(out, dlp + 1, (size_t)rows * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Test hook: the sampler's launches (three, or the whole-vocabulary six) on `rows` host rows of n_vocab logits, row r at sequence
// index positions[r]; the same kernels, scratch and device parameter struct as the engine's step.
extern "C" int gemma_test_sample(const float *logits, int rows, int n_vocab, const gemma_sampler *sp, const int32_t *positions,
                                 int32_t *tokens, int32_t *cand, int32_t *n_cand, int32_t *n_kept) {
    set_error("");
    if (!logits || !sp || !positions || rows <= 0) {
        set_error("gemma_test_sample: logits, sampler, positions and rows >= 1 are required");
        return -1;
    }
    if (n_vocab <= 0) {
        set_error("gemma_test_sample: n_vocab must be >= 1");
        return -1;
    }
    std::string why = sampler_invalid(*sp, n_vocab);
    if (why.empty() && !(sp->temperature > 0.0f)) why = "temperature must be > 0 (the sampler is off otherwise)";
    for (int r = 0; why.empty() && r < rows; ++r)
        if (positions[r] < 0 || positions[r] == INT32_MAX) why = "positions must be in [0, 2^31 - 1)";
    if (!why.empty()) {
        set_error("gemma_test_sample: " + why);
        return -1;
    }
    dev_pool tmp;
    sample_ws ws;
    sampler_params hp, *dp = nullptr;
    hp.temperature = sp->temperature; hp.top_k = sp->top_k; hp.top_p = sp->top_p; hp.seed = sp->seed;
    float *dl = nullptr;
    int *dpos = nullptr, *dtok = nullptr, *dcand = nullptr, *dnc = nullptr, *dnk = nullptr;
    std::vector<int> pm1(positions, positions + rows);
    for (int &v : pm1) v -= 1;  // the kernels read *pos + 1, as k_advance does
    const size_t row_b = (size_t)n_vocab * 4;
    // the batched launches: up to 64 rows a time, each row in its own workspace
    const int chunk = std::min(rows, (int)PICK_MAX_ROWS);
    if (sample_ws_alloc(tmp, &ws, n_vocab, nullptr, chunk)) return -1;
    if (tmp.get(&dp, sizeof(hp)) || tmp.get(&dl, row_b * rows) || tmp.get(&dpos, (size_t)rows * 4) ||
        tmp.get(&dtok, (size_t)rows * 4) || tmp.get(&dnc, (size_t)rows * 4) || tmp.get(&dnk, (size_t)rows * 4) ||
        tmp.get(&dcand, (size_t)rows * SAMPLE_MAX_K * 4))
        return -1;
    GHIP_CHECK(hipMemcpy(dp, &hp, sizeof(hp), hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dl, logits, row_b * rows, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dpos, pm1.data(), (size_t)rows * 4, hipMemcpyHostToDevice));
    for (int r = 0; r < rows; r += chunk) {
        sample_dbg d;
        d.token = dtok + r; d.cand = dcand + (size_t)r * SAMPLE_MAX_K; d.n_cand = dnc + r; d.n_kept = dnk + r;
        if (launch_sample(dl + (size_t)r * n_vocab, n_vocab, std::min(chunk, rows - r), n_vocab, dp, dpos + r, nullptr, ws, d, nullptr,
                          sampler_full(*sp) ? PICKS_FULL : PICKS_TRUNC))
            return -1;
    }
    GHIP_CHECK(hipDeviceSynchronize());
    if (tokens) GHIP_CHECK(hipMemcpy(tokens, dtok, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (n_cand) GHIP_CHECK(hipMemcpy(n_cand, dnc, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (n_kept) GHIP_CHECK(hipMemcpy(n_kept, dnk, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (cand) GHIP_CHECK(hipMemcpy(cand, dcand, (size_t)rows * SAMPLE_MAX_K * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Test hook: gemma_test_sample with one sampler per row, through launch_picks: the launches a batch
// pass takes for this mix of rows (picks_mix: the row argmax when some row is greedy, and each sampler's
// set of launches that some row needs).
// Every row's token is its pick key reduced as the advance kernels reduce it.
extern "C" int gemma_test_sample_rows(const float *logits, int rows, int n_vocab, const gemma_sampler *s_of,
                                      const int32_t *positions, int32_t *tokens, int32_t *cand, int32_t *n_cand,
                                      int32_t *n_kept) {
    set_error("");
    const std::string fn = "gemma_test_sample_rows";
    if (!logits || !s_of || !positions || rows <= 0 || n_vocab <= 0) {
        set_error(fn + ": logits, samplers, positions, rows >= 1 and n_vocab >= 1 are required");
        return -1;
    }
    int n_sample = 0, n_full = 0;
    for (int r = 0; r < rows; ++r) {
        std::string why = sampler_invalid(s_of[r], n_vocab);
        if (why.empty() && (positions[r] < 0 || positions[r] == INT32_MAX)) why = "positions must be in [0, 2^31 - 1)";
        if (!why.empty()) {
            set_error(fn + ": row " + std::to_string(r) + ": " + why);
            return -1;
        }
        n_sample += s_of[r].temperature > 0.0f;
        n_full += sampler_full(s_of[r]);
    }
    const int mix = picks_mix(rows, n_sample, n_full);
    dev_pool tmp;
    sample_ws ws;
    const int chunk = std::min(rows, (int)PICK_MAX_ROWS);
    const size_t row_b = (size_t)n_vocab * 4, n_keys = (size_t)chunk * 256 + chunk;
    slot_row *dtab = nullptr;
    float *dl = nullptr;
    int *dpos = nullptr, *dcand = nullptr, *dnc = nullptr, *dnk = nullptr;
    unsigned long long *dkeys = nullptr;
    if (mix != PICKS_GREEDY && sample_ws_alloc(tmp, &ws, n_vocab, nullptr, chunk)) return -1;
    if (tmp.get(&dtab, (size_t)rows * sizeof(slot_row)) ||
        tmp.get(&dl, row_b * rows) || tmp.get(&dpos, (size_t)rows * 4) ||
        tmp.get(&dnc, (size_t)rows * 4) || tmp.get(&dnk, (size_t)rows * 4) ||
        tmp.get(&dcand, (size_t)rows * SAMPLE_MAX_K * 4) || tmp.get(&dkeys, n_keys * 8))
        return -1;
    std::vector<slot_row> htab(rows);
    std::vector<int> pm1(positions, positions + rows);
    for (int r = 0; r < rows; ++r) {
        sampler_params &p = htab[r].smp;
        p.temperature = s_of[r].temperature; p.top_k = s_of[r].top_k; p.top_p = s_of[r].top_p; p.seed = s_of[r].seed;
        pm1[r] -= 1;  // the kernels read *pos + 1, as k_advance does
        htab[r].pos = dpos + r;
    }
    GHIP_CHECK(hipMemcpy(dtab, htab.data(), (size_t)rows * sizeof(slot_row), hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dl, logits, row_b * rows, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(dpos, pm1.data(), (size_t)rows * 4, hipMemcpyHostToDevice));
    // a greedy row writes no debug output: n_cand = n_kept = 0 and cand = -1 stand
    GHIP_CHECK(hipMemset(dnc, 0, (size_t)rows * 4));
    GHIP_CHECK(hipMemset(dnk, 0, (size_t)rows * 4));
    GHIP_CHECK(hipMemset(dcand, 0xFF, (size_t)rows * SAMPLE_MAX_K * 4));
    std::vector<unsigned long long> hk(n_keys);
    for (int r = 0; r < rows; r += chunk) {
        const int T = std::min(chunk, rows - r);
        sample_dbg d;
        d.cand = dcand + (size_t)r * SAMPLE_MAX_K; d.n_cand = dnc + r; d.n_kept = dnk + r;
        const unsigned long long *keys = nullptr;
        int n_parts = 0, stride = 0;
        if (launch_picks(mix, dl + (size_t)r * n_vocab, n_vocab, T, n_vocab, nullptr, nullptr, dtab + r, ws, dkeys, chunk, d,
                         nullptr, &keys, &n_parts, &stride))
            return -1;
        GHIP_CHECK(hipDeviceSynchronize());
        GHIP_CHECK(hipMemcpy(hk.data(), keys, ((size_t)(T - 1) * stride + n_parts) * 8, hipMemcpyDeviceToHost));
        for (int t = 0; tokens && t < T; ++t) {  // the maximum key's index: block_max_key, key_index (pick.h)
            unsigned long long best = 0;
            for (int i = 0; i < n_parts; ++i) best = std::max(best, hk[(size_t)t * stride + i]);
            tokens[r + t] = (int32_t)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull));
        }
    }
    if (n_cand) GHIP_CHECK(hipMemcpy(n_cand, dnc, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (n_kept) GHIP_CHECK(hipMemcpy(n_kept, dnk, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (cand) GHIP_CHECK(hipMemcpy(cand, dcand, (size_t)rows * SAMPLE_MAX_K * 4, hipMemcpyDeviceToHost));
    return 0;
}

// attention + attn-out in one launch on (1) / off (0) / unchanged (-1); returns the setting
extern "C" int gemma_engine_set_att_o(gemma_engine *e, int on) {
    if (on >= 0 && (on != 0) != (e->att_o != 0)) {
        e->att_o = on != 0 && e->ao_cnt;
        drop_graph(e);
    }
    return e->att_o;
}

// fused layer front on/off (tests, A/B); returns the sticky hand-off timeout word (0 = none seen)
extern "C" int gemma_engine_set_fuse(gemma_engine *e, int fuse_front) {
    if (fuse_front >= 0) {
        e->fuse_front = fuse_front;
        drop_graph(e);
    }
    int err = 0;
    if (e->front_err) (void)hipMemcpy(&err, e->front_err, 4, hipMemcpyDeviceToHost);
    return err;
}

extern "C" int gemma_engine_set_plan(gemma_engine *e, const int *in, int n) {
    const gemma_hip_config &c = e->cfg;
    const layer_dev &L0 = e->layers[0];
    const int64_t nbt[MC_N] = {L0.qkv.n_bt, L0.o.n_bt, L0.gate.n_bt, L0.down.n_bt, e->embd.n_bt};
    for (int cls = 0; cls < MC_N && 3 * cls + 2 < n; ++cls) {
        const int ks = in[3 * cls], rpw = in[3 * cls + 1], img = in[3 * cls + 2];
        const bool splits = cls == MC_QKV || cls == MC_O || cls == MC_DOWN || cls == MC_GU;
        const bool img_ok = (cls == MC_O && e->att_act) || (cls == MC_DOWN && e->h_act);
        if (ks < 1 || (!splits && ks != 1) || (cls == MC_GU && ks > 2) || pick_ks(c.wtype, nbt[cls], ks) != ks || rpw < 1 || rpw > 64 ||
            (img && !img_ok)) {
            set_error("gemma_engine_set_plan: infeasible plan");
            return -1;
        }
        e->plan[cls] = {ks, rpw, img ? 1 : 0};
    }
    if (n > 3 * MC_N) {
        const int mode = in[3 * MC_N];
        if ((mode != ATTN_PER_HEAD && mode != ATTN_SPLIT) || (mode == ATTN_SPLIT && !e->ag.nwg) ||
            (mode == ATTN_PER_HEAD && (c.head_dim > 256 || c.n_ctx > 2048))) {
            set_error("gemma_engine_set_plan: infeasible attention form");
            return -1;
        }
        e->att_mode = mode;
    }
    drop_graph(e);
    return 0;
}
// Diagnostic: one eager decode step with s_memrealtime phase stamps (100 MHz) for the five kernels
// of `layer` (regions 0..4: qkv, attention, o, gate/up, down) and the logits kernel (region 5).
// out: 6 * 4096 * 16 u64; unused slots are 0.
extern "C" int gemma_engine_stamp_step(gemma_engine *e, int layer, unsigned long long *out) {
    set_error("");
    if (!GHIP_STAMPS) {
        set_error("gemma_engine_stamp_step: library built without -DGHIP_STAMPS=1 (scripts/build_variant.sh)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    const size_t n = 6 * kStampRegion;
    dev_pool tmp;
    if (tmp.get_zeroed(&e->stamp, n * 8, e->stream)) return -1;
    e->stamp_layer = layer;
    auto run = [&]() -> int {
        if (enqueue_step(e)) return -1;
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        GHIP_CHECK(hipMemcpy(out, e->stamp, n * 8, hipMemcpyDeviceToHost));
        e->seq.host_pos += 1;
        return 0;
    };
    const int r = run();
    e->stamp = nullptr;  // on every exit: the buffer goes with tmp
    e->stamp_layer = -1;
    return r;
}

// diagnostics: one eager step through the persistent token launch with its phase stamps
// (s_memrealtime, 100 MHz) -> out [grid = n_embd / 8][n_layer][16]; needs a -DGHIP_STAMPS=1 build
// of token.hip and engine_diag.cpp (scripts/build_variant.sh)
extern "C" int gemma_engine_token_stamps(gemma_engine *e, unsigned long long *out) {
    set_error("");
    if (!GHIP_STAMPS) {
        set_error("gemma_engine_token_stamps: library built without -DGHIP_STAMPS=1 (scripts/build_variant.sh)");
        return -1;
    }
    (void)hipSetDevice(e->device);
    if (!persist_on(e)) {
        set_error("gemma_engine_token_stamps: the persistent launch is not active: " + e->persist_why);
        return -1;
    }
    const size_t n = (size_t)(e->cfg.n_embd / 8) * e->cfg.n_layer * 16 + 256;  // + per-pop probes
    unsigned long long *buf = nullptr;
    GHIP_CHECK(hipStreamSynchronize(e->stream));
    dev_pool tmp;
    if (tmp.get(&buf, n * 8)) return -1;
    GHIP_CHECK(hipMemset(buf, 0, n * 8));
    tok_args a = e->tok;
    a.dbg_t = buf;
    GHIP_CHECK(hipMemcpy(e->tok_dev, &a, sizeof(a), hipMemcpyHostToDevice));
    const int r = enqueue_step(e);
    const hipError_t se = hipStreamSynchronize(e->stream);
    // back to the plain arguments before anything can return: buf goes with tmp
    GHIP_CHECK(hipMemcpy(e->tok_dev, &e->tok, sizeof(e->tok), hipMemcpyHostToDevice));
    GHIP_CHECK(se);
    if (r == 0) {
        GHIP_CHECK(hipMemcpy(out, buf, n * 8, hipMemcpyDeviceToHost));
        e->seq.host_pos += 1;
    }
    return r;
}

// one eager step with per-layer taps copied to host: [L][qkv | attn | x_out]
extern "C" int gemma_engine_debug_step(gemma_engine *e, float *host_taps, float *logits) {
    set_error("");
    (void)hipSetDevice(e->device);
    const gemma_hip_config &c = e->cfg;
    const size_t per = (size_t)e->qkv_rows + e->qw + c.n_embd;
    dev_pool tmp;
    if (tmp.get(&e->dbg, per * c.n_layer * 4)) return -1;
    auto run = [&]() -> int {
        const int r = enqueue_step(e);
        GHIP_CHECK(hipStreamSynchronize(e->stream));
        if (r) return r;
        GHIP_CHECK(hipMemcpy(host_taps, e->dbg, per * c.n_layer * 4, hipMemcpyDeviceToHost));
        if (logits) GHIP_CHECK(hipMemcpy(logits, e->logits, (size_t)c.n_vocab * 4, hipMemcpyDeviceToHost));
        e->seq.host_pos += 1;
        return 0;
    };
    const int r = run();
    e->dbg = nullptr;  // on every exit (persist_on() is false while it is set); the buffer goes with tmp
    return r;
}

// ---- per-op test entry: the decode attention kernel on host buffers ---------------------------
// qkv [H*hd + 2*Hkv*hd] f32; kc [ctx][Hkv*hd], vc [Hkv*hd][ctx] f16 (updated in place at pos)
extern "C" int gemma_test_attn_decode(const float *qkv, uint16_t *kc, uint16_t *vc, int pos, int H, int Hkv, int hd,
                                      int ctx, float rope_base, float *out, float *dbg_w, uint16_t *dbg_p,
                                      float *dbg_inv, unsigned long long *dbg_t, int mode) {
    set_error("");
    const size_t qkv_n = (size_t)(H + 2 * Hkv) * hd, cache_n = (size_t)ctx * Hkv * hd;
    std::vector<uint16_t> et, gt;
    build_f16_tables(et, gt);
    std::vector<float> rc, rs;
    build_rope(ctx, hd, rope_base, rc, rs);
    dev_pool tmp;
    float *d_qkv, *d_out, *d_c, *d_s;
    uint16_t *d_k, *d_v, *d_e;
    int *d_pos;
    float *d_dw = nullptr, *d_di = nullptr;
    unsigned long long *d_dt = nullptr;
    const size_t n_stamps = (size_t)H * 8 * 8;  // >= workgroups x 8 stamps for any hd <= 512
    if (dbg_t && tmp.get(&d_dt, n_stamps * 8)) return -1;
    if (dbg_t) GHIP_CHECK(hipMemset(d_dt, 0, n_stamps * 8));
    uint16_t *d_dp = nullptr;
    if (dbg_w && tmp.get(&d_dw, (size_t)H * ctx * 4)) return -1;
    if (dbg_p && tmp.get(&d_dp, (size_t)H * ctx * 2)) return -1;
    if (dbg_inv && tmp.get(&d_di, (size_t)H * 4)) return -1;
    if (tmp.get(&d_qkv, qkv_n * 4)) return -1;
    if (tmp.get(&d_out, (size_t)H * hd * 4)) return -1;
    if (tmp.get(&d_c, rc.size() * 4)) return -1;
    if (tmp.get(&d_s, rs.size() * 4)) return -1;
    if (tmp.get(&d_k, cache_n * 2)) return -1;
    if (tmp.get(&d_v, cache_n * 2)) return -1;
    if (tmp.get(&d_e, 65536 * 2)) return -1;
    if (tmp.get(&d_pos, 4)) return -1;
    GHIP_CHECK(hipMemcpy(d_qkv, qkv, qkv_n * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_c, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_e, et.data(), 65536 * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_pos, &pos, 4, hipMemcpyHostToDevice));
    const attn_geom g = attn_geometry(H, Hkv, hd, ctx);
    float *d_sb = nullptr;
    int *d_sy = nullptr;
    if (g.nwg) {
        if (tmp.get(&d_sb, g.sbuf_floats * 4)) return -1;
        if (tmp.get(&d_sy, (g.sync_ints + 1) * 4)) return -1;
        GHIP_CHECK(hipMemset(d_sy, 0, (g.sync_ints + 1) * 4));
    }
    attn_args a;
    a.qkv = d_qkv; a.kc = d_k; a.vc = d_v; a.rope_cos = d_c; a.rope_sin = d_s; a.exp_tab = d_e; a.pos = d_pos;
    a.nwg = g.nwg; a.sbuf = d_sb; a.sync = d_sy; a.err = d_sy ? d_sy + g.sync_ints : nullptr;
    float *d_rc = nullptr;
    if (tmp.get(&d_rc, (size_t)(hd + 4) * 4)) return -1;
    GHIP_CHECK(hipMemcpy(d_rc, rc.data() + (size_t)pos * (hd / 2), (size_t)(hd / 2) * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rc + hd / 2, rs.data() + (size_t)pos * (hd / 2), (size_t)(hd / 2) * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rc + hd, &pos, 4, hipMemcpyHostToDevice));
    a.rope_cur = d_rc;
    // mode 0 per-head, 1 split form; 2 / 3: per-head with 2 / 4 workgroups per head (dim split)
    a.mode = mode >= 2 ? ATTN_PER_HEAD : mode;
    a.dsplit = mode == 2 ? 2 : mode == 3 ? 4 : 1;
    a.out = d_out; a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.q_scale = 1.0f / sqrtf((float)hd);
    a.dbg_w = d_dw; a.dbg_p = d_dp; a.dbg_inv = d_di; a.dbg_t = d_dt;
    int r = 0;
    for (int rep = 0; rep < (dbg_t ? 3 : 1) && r == 0; ++rep) r = launch_attn_decode(a, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) {
        GHIP_CHECK(hipMemcpy(out, d_out, (size_t)H * hd * 4, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(kc, d_k, cache_n * 2, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(vc, d_v, cache_n * 2, hipMemcpyDeviceToHost));
        if (dbg_w) GHIP_CHECK(hipMemcpy(dbg_w, d_dw, (size_t)H * ctx * 4, hipMemcpyDeviceToHost));
        if (dbg_p) GHIP_CHECK(hipMemcpy(dbg_p, d_dp, (size_t)H * ctx * 2, hipMemcpyDeviceToHost));
        if (dbg_inv) GHIP_CHECK(hipMemcpy(dbg_inv, d_di, (size_t)H * 4, hipMemcpyDeviceToHost));
        if (dbg_t) GHIP_CHECK(hipMemcpy(dbg_t, d_dt, n_stamps * 8, hipMemcpyDeviceToHost));
    }
    if (r == 0 && d_sy) {
        int err = 0;
        GHIP_CHECK(hipMemcpy(&err, d_sy + g.sync_ints, 4, hipMemcpyDeviceToHost));
        if (err) {
            set_error("attn_decode: hand-off spin timed out");
            r = -1;
        }
    }
    return r;
}

// ---- per-op test entries: the prefill attention's kernels, each alone, on host buffers ----------
// qkv [T][ldqkv] f32 rows q | k | v (pre-RoPE) of positions p0 .. p0 + T - 1; q16_out [T][H][hd] f16;
// kc_inout [ctx][Hkv*hd], vc_inout [Hkv*hd][ctx] f16 (rows / columns p0 .. p0 + T - 1 written)
extern "C" int gemma_test_rope_kv_prefill(const float *qkv, int64_t ldqkv, int T, int p0, int H, int Hkv, int hd, int ctx,
                                          float rope_base, uint16_t *q16_out, uint16_t *kc_inout, uint16_t *vc_inout) {
    set_error("");
    if (!qkv || !q16_out || !kc_inout || !vc_inout || T <= 0 || p0 < 0 || H <= 0 || Hkv <= 0 || hd <= 0 || hd % 2 ||
        hd > 1024 || ctx <= 0 || p0 + T > ctx || ldqkv < (int64_t)(H + 2 * Hkv) * hd) {
        set_error("gemma_test_rope_kv_prefill: bad arguments (rows p0 .. p0 + T - 1 inside ctx, ldqkv >= (H + 2 Hkv) hd)");
        return -1;
    }
    const size_t in_n = (size_t)T * ldqkv, q_n = (size_t)T * H * hd, cache_n = (size_t)ctx * Hkv * hd;
    std::vector<float> rc, rs;
    build_rope(ctx, hd, rope_base, rc, rs);
    dev_pool tmp;
    float *d_qkv, *d_c, *d_s;
    uint16_t *d_q, *d_k, *d_v;
    if (tmp.get(&d_qkv, in_n * 4) || tmp.get(&d_c, rc.size() * 4) || tmp.get(&d_s, rs.size() * 4) || tmp.get(&d_q, q_n * 2) ||
        tmp.get(&d_k, cache_n * 2) || tmp.get(&d_v, cache_n * 2))
        return -1;
    GHIP_CHECK(hipMemcpy(d_qkv, qkv, in_n * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_c, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_q, q16_out, q_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc_inout, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc_inout, cache_n * 2, hipMemcpyHostToDevice));
    ropekv_args a;
    a.qkv = d_qkv; a.ldqkv = ldqkv; a.rope_cos = d_c; a.rope_sin = d_s; a.q16 = d_q; a.kc = d_k; a.vc = d_v;
    a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.p0 = p0; a.q_scale = 1.0f / sqrtf((float)hd);
    const int r = launch_rope_kv_prefill(a, T, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) {
        GHIP_CHECK(hipMemcpy(q16_out, d_q, q_n * 2, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(kc_inout, d_k, cache_n * 2, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(vc_inout, d_v, cache_n * 2, hipMemcpyDeviceToHost));
    }
    return r;
}

// the same rows' K / V store through k_rows_rope_kv (batch.hip), which restates k_rope_kv_prefill for a
// pass's row table: one slot_row per row, all on the same caches, the row's position in its RoPE row's word
extern "C" int gemma_test_rows_rope_kv(const float *qkv, int64_t ldqkv, int T, int p0, int H, int Hkv, int hd, int ctx,
                                       float rope_base, uint16_t *kc_inout, uint16_t *vc_inout) {
    set_error("");
    if (!qkv || !kc_inout || !vc_inout || T <= 0 || T > ATTN_SLOTS_MAX_R || p0 < 0 || H <= 0 || Hkv <= 0 || hd <= 0 ||
        hd % 2 || hd > 1024 || ctx <= 0 || p0 + T > ctx || ldqkv < (int64_t)(H + 2 * Hkv) * hd) {
        set_error("gemma_test_rows_rope_kv: bad arguments (1 .. 64 rows p0 .. p0 + T - 1 inside ctx, ldqkv >= (H + 2 Hkv) hd)");
        return -1;
    }
    const size_t in_n = (size_t)T * ldqkv, cache_n = (size_t)ctx * Hkv * hd, rw = (size_t)hd + 4;
    std::vector<float> rc, rs;
    build_rope(ctx, hd, rope_base, rc, rs);
    dev_pool tmp;
    float *d_qkv, *d_c, *d_s, *d_rope;
    uint16_t *d_k, *d_v;
    slot_row *d_rows;
    if (tmp.get(&d_qkv, in_n * 4) || tmp.get(&d_c, rc.size() * 4) || tmp.get(&d_s, rs.size() * 4) ||
        tmp.get(&d_rope, T * rw * 4) || tmp.get(&d_k, cache_n * 2) || tmp.get(&d_v, cache_n * 2) ||
        tmp.get(&d_rows, (size_t)T * sizeof(slot_row)))
        return -1;
    std::vector<float> rope(T * rw, 0.0f);
    std::vector<slot_row> rows(T);
    for (int t = 0; t < T; ++t) {
        const int p = p0 + t;
        memcpy(&rope[t * rw], rc.data() + (size_t)p * (hd / 2), (size_t)(hd / 2) * 4);
        memcpy(&rope[t * rw + hd / 2], rs.data() + (size_t)p * (hd / 2), (size_t)(hd / 2) * 4);
        memcpy(&rope[t * rw + hd], &p, 4);
        rows[t].qkv = d_qkv + (size_t)t * ldqkv;
        rows[t].kc = d_k;
        rows[t].vc = d_v;
        rows[t].rope = d_rope + t * rw;
    }
    GHIP_CHECK(hipMemcpy(d_qkv, qkv, in_n * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_c, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rope, rope.data(), rope.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc_inout, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc_inout, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rows, rows.data(), (size_t)T * sizeof(slot_row), hipMemcpyHostToDevice));
    attn_args a{};
    a.rope_cos = d_c; a.rope_sin = d_s; a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.q_scale = 1.0f / sqrtf((float)hd);
    const int r = launch_rows_rope_kv(a, d_rows, T, 0, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) {
        GHIP_CHECK(hipMemcpy(kc_inout, d_k, cache_n * 2, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(vc_inout, d_v, cache_n * 2, hipMemcpyDeviceToHost));
    }
    return r;
}

// the context shift's two cache launches (kv_shift.hip) on one layer's images, whole in and whole out; the RoPE row
// of position `discard` is the last row of the engine's table builder
extern "C" int gemma_test_kv_shift(uint16_t *kc_inout, uint16_t *vc_inout, int ctx, int Hkv, int hd, int pos, int keep,
                                   int discard, float rope_base) {
    set_error("");
    if (!kc_inout || !vc_inout || ctx <= 0 || Hkv <= 0 || hd <= 0 || hd % 2 || discard < 1 || discard >= ctx) {
        set_error("gemma_test_kv_shift: bad arguments (images, shapes, 1 <= discard < ctx)");
        return -1;
    }
    const size_t cache_n = (size_t)ctx * Hkv * hd, half = (size_t)hd / 2;
    std::vector<float> rc, rs;
    build_rope(discard + 1, hd, rope_base, rc, rs);
    dev_pool tmp;
    float *d_c, *d_s;
    uint16_t *d_k, *d_v;
    if (tmp.get(&d_c, half * 4) || tmp.get(&d_s, half * 4) || tmp.get(&d_k, cache_n * 2) || tmp.get(&d_v, cache_n * 2)) return -1;
    GHIP_CHECK(hipMemcpy(d_c, rc.data() + (size_t)discard * half, half * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data() + (size_t)discard * half, half * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc_inout, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc_inout, cache_n * 2, hipMemcpyHostToDevice));
    kv_shift_args a;
    a.kc = d_k; a.vc = d_v; a.n_layer = 1; a.layer_stride = (int64_t)cache_n; a.ctx = ctx; a.Hkv = Hkv; a.hd = hd;
    a.pos = pos; a.keep = keep; a.discard = discard; a.cs = d_c; a.sn = d_s;
    const int r = launch_kv_shift(a, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) {
        GHIP_CHECK(hipMemcpy(kc_inout, d_k, cache_n * 2, hipMemcpyDeviceToHost));
        GHIP_CHECK(hipMemcpy(vc_inout, d_v, cache_n * 2, hipMemcpyDeviceToHost));
    }
    return r;
}

// q16 [T][H][hd], kc [ctx][Hkv*hd], vc [Hkv*hd][ctx] f16; out [T][ldo] f32, copied in before the launch
// and back after it (columns past H*hd keep what the caller put there).  form 0 k_attn_rows, 1 k_attn_mx,
// 2 k_attn_prefill; a shape the form's launcher refuses: non-zero with its message, out untouched
extern "C" int gemma_test_attn_prefill(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, int T, int p0, int H,
                                       int Hkv, int hd, int ctx, int n_kv, int64_t ldo, int form, float *out) {
    set_error("");
    if (!q16 || !kc || !vc || !out || T <= 0 || p0 < 0 || H <= 0 || Hkv <= 0 || hd <= 0 || ctx <= 0 || n_kv <= 0 ||
        ldo < (int64_t)H * hd || form < 0 || form > 2) {
        set_error("gemma_test_attn_prefill: bad arguments (form 0 rows, 1 mx, 2 f16 MFMA; ldo >= H * hd)");
        return -1;
    }
    const size_t q_n = (size_t)T * H * hd, cache_n = (size_t)ctx * Hkv * hd, out_n = (size_t)T * ldo;
    dev_pool tmp;
    uint16_t *d_q, *d_k, *d_v;
    float *d_out;
    // (the kernels' 16-byte reads stay inside a row; the allocator's granule covers nothing else)
    if (tmp.get(&d_q, q_n * 2) || tmp.get(&d_k, cache_n * 2) || tmp.get(&d_v, cache_n * 2) || tmp.get(&d_out, out_n * 4))
        return -1;
    GHIP_CHECK(hipMemcpy(d_q, q16, q_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_out, out, out_n * 4, hipMemcpyHostToDevice));
    attnp_args a;
    a.q16 = d_q; a.kc = d_k; a.vc = d_v; a.out = d_out; a.ldo = ldo;
    a.T = T; a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.n_kv = n_kv; a.p0 = p0;
    if (form == 2 && (H % Hkv || n_kv > ctx || p0 + T > n_kv)) {  // (launch_attn_prefill checks the head shape only)
        set_error("attn_prefill: unsupported shape (rows p0 .. p0 + T - 1 inside n_kv <= ctx)");
        return -1;
    }
    const int r = form == 0 ? launch_attn_rows(a, nullptr) : form == 1 ? launch_attn_mx(a, nullptr) : launch_attn_prefill(a, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) GHIP_CHECK(hipMemcpy(out, d_out, out_n * 4, hipMemcpyDeviceToHost));
    return r;
}

// the same rows through the key-split matrix-core form (attn_mx_long.hip) as ONE call of its launcher.  Its
// scratch goes in as a pass would find it after earlier ones, only worse: large finite words, so a stale word
// that a kernel reads wins the max and changes the output
extern "C" int gemma_test_attn_mx_long(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, int T, int p0, int H,
                                       int Hkv, int hd, int ctx, int n_kv, int64_t ldo, float *out) {
    set_error("");
    if (!q16 || !kc || !vc || !out || T <= 0 || p0 < 0 || H <= 0 || Hkv <= 0 || hd <= 0 || ctx <= 0 || n_kv <= 0 ||
        ldo < (int64_t)H * hd) {
        set_error("gemma_test_attn_mx_long: bad arguments (ldo >= H * hd)");
        return -1;
    }
    attnp_args a;
    a.ldo = ldo; a.T = T; a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.n_kv = n_kv; a.p0 = p0;
    if (const char *why = attn_mx_long_unsupported(a)) {  // before anything is sized by the shape
        set_error(std::string("attn_mx_long: ") + why);
        return -1;
    }
    const size_t q_n = (size_t)T * H * hd, cache_n = (size_t)ctx * Hkv * hd, out_n = (size_t)T * ldo;
    const int slab_rows = attn_mx_long_slab_rows(T);
    const size_t sb_n = attn_mx_long_scratch(slab_rows, H, ctx, false) / 4;
    dev_pool tmp;
    uint16_t *d_q, *d_k, *d_v, *d_pb;
    float *d_out, *d_sb;
    if (tmp.get(&d_q, q_n * 2) || tmp.get(&d_k, cache_n * 2) || tmp.get(&d_v, cache_n * 2) || tmp.get(&d_out, out_n * 4) ||
        tmp.get(&d_sb, sb_n * 4) || tmp.get(&d_pb, sb_n * 2))
        return -1;
    {
        std::vector<float> sb(sb_n, GEMMA_TEST_ATTN_LONG_W_FILL);
        std::vector<uint16_t> pb(sb_n, (uint16_t)GEMMA_TEST_ATTN_LONG_P_FILL);
        GHIP_CHECK(hipMemcpy(d_sb, sb.data(), sb_n * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(d_pb, pb.data(), sb_n * 2, hipMemcpyHostToDevice));
    }
    GHIP_CHECK(hipMemcpy(d_q, q16, q_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, kc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, vc, cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_out, out, out_n * 4, hipMemcpyHostToDevice));
    a.q16 = d_q; a.kc = d_k; a.vc = d_v; a.out = d_out;
    const int r = launch_attn_mx_long(a, d_sb, d_pb, slab_rows, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r == 0) GHIP_CHECK(hipMemcpy(out, d_out, out_n * 4, hipMemcpyDeviceToHost));
    return r;
}

// ---- per-op test entry: the decode attention's launch forms, R rows on host buffers (include/gemma_hpc.h) ----
extern "C" int gemma_test_attn_decode_rows(gemma_test_attn_rows_args *t) {
    set_error("");
    if (!t) {
        set_error("gemma_test_attn_decode_rows: no arguments");
        return -1;
    }
    t->err_out = 0;
    const int form = t->form, R = t->R, H = t->H, Hkv = t->Hkv, hd = t->hd, ctx = t->ctx;
    if (form < 0 || form > 3 || R < 0 || R > 1024 || (form < 2 && R < 1) || t->n_slots < 1 || t->n_slots > 1024 || H <= 0 ||
        H > 256 || Hkv <= 0 || Hkv > 256 || hd <= 0 || hd % 8 || hd > 1024 || ctx <= 0 || ctx % 8 || ctx > (1 << 20) ||
        !t->qkv || t->ldqkv < (int64_t)(H + 2 * Hkv) * hd || t->ldqkv % 4 || !t->pos || !t->slot || !t->kc || !t->vc ||
        !t->out || !t->img_act != !t->img_da || t->dsplit < 0 || t->nwg < 0) {
        set_error("gemma_test_attn_decode_rows: bad arguments (form 0 .. 3; forms 0 / 1 need R >= 1; head_dim and ctx "
                  "multiples of 8; ldqkv >= (H + 2 Hkv) hd, a multiple of 4; img_act and img_da together)");
        return -1;
    }
    for (int r = 0; r < R; ++r)
        if (t->pos[r] < 0 || t->pos[r] >= ctx || t->slot[r] < 0 || t->slot[r] >= t->n_slots) {
            set_error("gemma_test_attn_decode_rows: a row's position outside [0, ctx) or its slot outside [0, n_slots)");
            return -1;
        }
    if (form >= 2 && R > 1 && (t->dbg_w || t->dbg_p)) {
        set_error("gemma_test_attn_decode_rows: the taps are indexed by head only: forms 2 and 3 take them for R == 1");
        return -1;
    }
    if (form == 2)
        for (int r = 0; r < R; ++r)
            for (int q = 0; q < r; ++q)
                if (t->slot[q] == t->slot[r]) {
                    set_error("gemma_test_attn_decode_rows: form 2 needs a distinct slot per row");
                    return -1;
                }
    // form 3: the rows of a slot adjacent and at consecutive positions; (off, rank) as the engine's planner numbers them
    std::vector<int> off(std::max(R, 1), 0), rank(std::max(R, 1), 0), first(std::max(R, 1), 0);
    if (form == 3)
        for (int r = 0, n_rank = 0; r < R; ++r) {
            if (r > 0 && t->slot[r] == t->slot[r - 1]) {
                off[r] = off[r - 1] + 1;
                rank[r] = rank[r - 1];
                first[r] = first[r - 1];
                if (t->pos[r] != t->pos[r - 1] + 1) {
                    set_error("gemma_test_attn_decode_rows: form 3 needs a slot's rows at consecutive positions");
                    return -1;
                }
            } else {
                for (int q = 0; q < r; ++q)
                    if (t->slot[q] == t->slot[r]) {
                        set_error("gemma_test_attn_decode_rows: form 3 needs the rows of a slot adjacent");
                        return -1;
                    }
                rank[r] = n_rank++;
                first[r] = r;
            }
        }
    const int Rn = std::max(R, 1);
    const size_t qkv_n = (size_t)(R > 0 ? (R - 1) * t->ldqkv + (int64_t)(H + 2 * Hkv) * hd : 4), cache_n = (size_t)ctx * Hkv * hd;
    const size_t out_n = (size_t)Rn * H * hd, tap_n = (size_t)Rn * H * ctx, rw = (size_t)hd + 4, half = (size_t)hd / 2;
    const size_t blocks = ((size_t)H * hd + 31) / 32, act_n = (blocks + 3) / 4 * 32, q8k_n = (size_t)H * 292;
    std::vector<uint16_t> et, gt;
    build_f16_tables(et, gt);
    std::vector<float> rc, rs;
    if (t->rope_identity) {
        rc.assign((size_t)ctx * half, 1.0f);
        rs.assign((size_t)ctx * half, 0.0f);
    } else {
        build_rope(ctx, hd, t->rope_base, rc, rs);
    }
    std::vector<float> rope(Rn * rw, 0.0f);
    for (int r = 0; r < R; ++r) {
        const int p = t->pos[r];
        memcpy(&rope[r * rw], rc.data() + (size_t)p * half, half * 4);
        memcpy(&rope[r * rw + half], rs.data() + (size_t)p * half, half * 4);
        memcpy(&rope[r * rw + hd], &p, 4);
    }
    const attn_geom g = attn_geometry(H, Hkv, hd, ctx);
    dev_pool tmp;
    float *d_qkv, *d_out, *d_c, *d_s, *d_rope, *d_dw = nullptr, *d_da = nullptr, *d_sb = nullptr;
    uint16_t *d_k, *d_v, *d_e, *d_dp = nullptr;
    uint32_t *d_act = nullptr;
    uint8_t *d_q8k = nullptr;
    int *d_pos, *d_sy = nullptr;
    slot_row *d_rows;
    row_src *d_src;
    const size_t sync_n = (size_t)Hkv * 2;
    if (tmp.get(&d_qkv, qkv_n * 4) || tmp.get(&d_out, out_n * 4) || tmp.get(&d_c, rc.size() * 4) || tmp.get(&d_s, rs.size() * 4) ||
        tmp.get(&d_rope, rope.size() * 4) || tmp.get(&d_k, (size_t)t->n_slots * cache_n * 2) ||
        tmp.get(&d_v, (size_t)t->n_slots * cache_n * 2) || tmp.get(&d_e, 65536 * 2) || tmp.get(&d_pos, (size_t)Rn * 4) ||
        tmp.get(&d_rows, (size_t)Rn * sizeof(slot_row)) || tmp.get(&d_src, (size_t)Rn * sizeof(row_src)))
        return -1;
    if (t->dbg_w && tmp.get(&d_dw, tap_n * 4)) return -1;
    if (t->dbg_p && tmp.get(&d_dp, tap_n * 2)) return -1;
    if (t->img_act && (tmp.get(&d_act, Rn * act_n * 4) || tmp.get(&d_da, Rn * blocks * 4))) return -1;
    if (t->img_q8k && tmp.get(&d_q8k, Rn * q8k_n)) return -1;
    if (form == 1) {
        if (tmp.get(&d_sb, std::max(g.sbuf_floats, (size_t)4) * 4) || tmp.get(&d_sy, (sync_n + 1) * 4)) return -1;
        GHIP_CHECK(hipMemset(d_sy, 0, (sync_n + 1) * 4));
    }
    if (R > 0) {
        GHIP_CHECK(hipMemcpy(d_qkv, t->qkv, qkv_n * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(d_out, t->out, out_n * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(d_pos, t->pos, (size_t)R * 4, hipMemcpyHostToDevice));
        if (d_dw) GHIP_CHECK(hipMemcpy(d_dw, t->dbg_w, tap_n * 4, hipMemcpyHostToDevice));
        if (d_dp) GHIP_CHECK(hipMemcpy(d_dp, t->dbg_p, tap_n * 2, hipMemcpyHostToDevice));
        if (d_act) GHIP_CHECK(hipMemcpy(d_act, t->img_act, R * act_n * 4, hipMemcpyHostToDevice));
        if (d_da) GHIP_CHECK(hipMemcpy(d_da, t->img_da, R * blocks * 4, hipMemcpyHostToDevice));
        if (d_q8k) GHIP_CHECK(hipMemcpy(d_q8k, t->img_q8k, R * q8k_n, hipMemcpyHostToDevice));
    }
    GHIP_CHECK(hipMemcpy(d_c, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rope, rope.data(), rope.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, t->kc, (size_t)t->n_slots * cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, t->vc, (size_t)t->n_slots * cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_e, et.data(), 65536 * 2, hipMemcpyHostToDevice));
    std::vector<slot_row> rows(Rn);
    std::vector<row_src> src(Rn);
    for (int r = 0; r < R; ++r) {
        rows[r].qkv = d_qkv + (size_t)r * t->ldqkv;
        rows[r].out = d_out + (size_t)r * H * hd;
        rows[r].kc = d_k + (size_t)t->slot[r] * cache_n;
        rows[r].vc = d_v + (size_t)t->slot[r] * cache_n;
        rows[r].rope = d_rope + r * rw;
        rows[r].pos = d_pos + r;
        src[r].spos = d_pos + first[r];  // the slot's position word: its first row's
        src[r].off = off[r];
        src[r].rank = rank[r];
    }
    GHIP_CHECK(hipMemcpy(d_rows, rows.data(), (size_t)Rn * sizeof(slot_row), hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_src, src.data(), (size_t)Rn * sizeof(row_src), hipMemcpyHostToDevice));
    attn_args a{};
    a.rope_cos = d_c; a.rope_sin = d_s; a.exp_tab = d_e;
    a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.q_scale = t->q_scale;
    a.mode = form == 1 ? ATTN_SPLIT : ATTN_PER_HEAD;
    a.dsplit = form == 1 ? 1 : t->dsplit;
    a.nwg = form == 1 ? (t->nwg ? t->nwg : g.nwg) : 0;
    a.sbuf = d_sb; a.sync = d_sy; a.err = d_sy ? d_sy + sync_n : nullptr;
    int r = 0;
    if (form < 2) {
        for (int i = 0; i < R && r == 0; ++i) {
            a.qkv = rows[i].qkv; a.kc = rows[i].kc; a.vc = rows[i].vc; a.rope_cur = rows[i].rope; a.pos = rows[i].pos;
            a.out = rows[i].out;
            a.dbg_w = d_dw ? d_dw + (size_t)i * H * ctx : nullptr;
            a.dbg_p = d_dp ? d_dp + (size_t)i * H * ctx : nullptr;
            a.out_act = d_act ? d_act + i * act_n : nullptr;
            a.out_da = d_da ? d_da + i * blocks : nullptr;
            a.out_q8k = d_q8k ? d_q8k + i * q8k_n : nullptr;
            r = launch_attn_decode(a, nullptr);
        }
    } else {
        a.dbg_w = d_dw; a.dbg_p = d_dp;
        a.out_act = d_act; a.out_da = d_da; a.out_q8k = d_q8k;  // (both launchers refuse an image)
        r = form == 2 ? launch_attn_slots(a, d_rows, R, 0, nullptr) : launch_attn_slot_rows(a, d_rows, d_src, R, 0, nullptr);
    }
    GHIP_CHECK(hipDeviceSynchronize());
    if (r != 0) return r;
    if (d_sy) {
        std::vector<int> sy(sync_n + 1);
        GHIP_CHECK(hipMemcpy(sy.data(), d_sy, (sync_n + 1) * 4, hipMemcpyDeviceToHost));
        if (t->sync_out) memcpy(t->sync_out, sy.data(), sync_n * 4);
        t->err_out = sy[sync_n];
    }
    GHIP_CHECK(hipMemcpy(t->out, d_out, out_n * 4, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(t->kc, d_k, (size_t)t->n_slots * cache_n * 2, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(t->vc, d_v, (size_t)t->n_slots * cache_n * 2, hipMemcpyDeviceToHost));
    if (d_dw) GHIP_CHECK(hipMemcpy(t->dbg_w, d_dw, tap_n * 4, hipMemcpyDeviceToHost));
    if (d_dp) GHIP_CHECK(hipMemcpy(t->dbg_p, d_dp, tap_n * 2, hipMemcpyDeviceToHost));
    if (d_act) GHIP_CHECK(hipMemcpy(t->img_act, d_act, R * act_n * 4, hipMemcpyDeviceToHost));
    if (d_da) GHIP_CHECK(hipMemcpy(t->img_da, d_da, R * blocks * 4, hipMemcpyDeviceToHost));
    if (d_q8k) GHIP_CHECK(hipMemcpy(t->img_q8k, d_q8k, R * q8k_n, hipMemcpyDeviceToHost));
    return 0;
}

// ---- per-op test entry: the long form of the batch pass's attention, R rows on host buffers (include/gemma_hpc.h) ----
extern "C" int gemma_test_attn_long_rows(gemma_test_attn_rows_args *t) {
    set_error("");
    const char *fn = "gemma_test_attn_long_rows";
    if (!t) {
        set_error(std::string(fn) + ": no arguments");
        return -1;
    }
    t->err_out = 0;
    const int R = t->R, H = t->H, Hkv = t->Hkv, hd = t->hd, ctx = t->ctx;
    if (t->form != 0 || R < 0 || R > 1024 || t->n_slots < 1 || t->n_slots > 1024 || H <= 0 || H > 256 || Hkv <= 0 || Hkv > 256 ||
        H % Hkv || hd <= 0 || hd % 8 || hd > 1024 || ctx <= 0 || ctx % 8 || ctx > (1 << 20) || !t->qkv ||
        t->ldqkv < (int64_t)(H + 2 * Hkv) * hd || t->ldqkv % 4 || !t->pos || !t->slot || !t->kc || !t->vc || !t->out ||
        !t->dbg_w || !t->dbg_p || t->img_act || t->img_da || t->img_q8k) {
        set_error(std::string(fn) + ": bad arguments (form 0; H a multiple of Hkv; head_dim and ctx multiples of 8; ldqkv >= "
                                    "(H + 2 Hkv) hd, a multiple of 4; dbg_w and dbg_p required; no image)");
        return -1;
    }
    for (int r = 0; r < R; ++r) {
        if (t->pos[r] < 0 || t->pos[r] >= ctx || t->slot[r] < 0 || t->slot[r] >= t->n_slots) {
            set_error(std::string(fn) + ": a row's position outside [0, ctx) or its slot outside [0, n_slots)");
            return -1;
        }
        for (int q = 0; q < r; ++q)
            if (t->slot[q] == t->slot[r] && t->pos[q] == t->pos[r]) {
                set_error(std::string(fn) + ": two rows of a slot at one position");
                return -1;
            }
    }
    const int Rn = std::max(R, 1), G = H / Hkv;
    const size_t qkv_n = (size_t)(R > 0 ? (R - 1) * t->ldqkv + (int64_t)(H + 2 * Hkv) * hd : 4), cache_n = (size_t)ctx * Hkv * hd;
    const size_t out_n = (size_t)Rn * H * hd, tap_n = (size_t)Rn * H * ctx, rw = (size_t)hd + 4, half = (size_t)hd / 2;
    std::vector<float> rc, rs;
    if (t->rope_identity) {
        rc.assign((size_t)ctx * half, 1.0f);
        rs.assign((size_t)ctx * half, 0.0f);
    } else {
        build_rope(ctx, hd, t->rope_base, rc, rs);
    }
    std::vector<float> rope(Rn * rw, 0.0f);
    for (int r = 0; r < R; ++r) {
        const int p = t->pos[r];
        memcpy(&rope[r * rw], rc.data() + (size_t)p * half, half * 4);
        memcpy(&rope[r * rw + half], rs.data() + (size_t)p * half, half * 4);
        memcpy(&rope[r * rw + hd], &p, 4);
    }
    dev_pool tmp;
    float *d_qkv, *d_out, *d_c, *d_s, *d_rope, *d_sb;
    uint16_t *d_k, *d_v, *d_pb;
    int *d_pos;
    slot_row *d_rows;
    if (tmp.get(&d_qkv, qkv_n * 4) || tmp.get(&d_out, out_n * 4) || tmp.get(&d_c, rc.size() * 4) || tmp.get(&d_s, rs.size() * 4) ||
        tmp.get(&d_rope, rope.size() * 4) || tmp.get(&d_k, (size_t)t->n_slots * cache_n * 2) ||
        tmp.get(&d_v, (size_t)t->n_slots * cache_n * 2) || tmp.get(&d_pos, (size_t)Rn * 4) ||
        tmp.get(&d_rows, (size_t)Rn * sizeof(slot_row)) || tmp.get(&d_sb, tap_n * 4) || tmp.get(&d_pb, tap_n * 2))
        return -1;
    // the form's scratch as a batch would hold it after earlier passes, only worse: large finite words
    std::vector<float> sb(tap_n, GEMMA_TEST_ATTN_LONG_W_FILL);
    std::vector<uint16_t> pb(tap_n, (uint16_t)GEMMA_TEST_ATTN_LONG_P_FILL);
    GHIP_CHECK(hipMemcpy(d_sb, sb.data(), tap_n * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_pb, pb.data(), tap_n * 2, hipMemcpyHostToDevice));
    if (R > 0) {
        GHIP_CHECK(hipMemcpy(d_qkv, t->qkv, qkv_n * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(d_out, t->out, out_n * 4, hipMemcpyHostToDevice));
        GHIP_CHECK(hipMemcpy(d_pos, t->pos, (size_t)R * 4, hipMemcpyHostToDevice));
    }
    GHIP_CHECK(hipMemcpy(d_c, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_s, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_rope, rope.data(), rope.size() * 4, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_k, t->kc, (size_t)t->n_slots * cache_n * 2, hipMemcpyHostToDevice));
    GHIP_CHECK(hipMemcpy(d_v, t->vc, (size_t)t->n_slots * cache_n * 2, hipMemcpyHostToDevice));
    std::vector<slot_row> rows(Rn);
    for (int r = 0; r < R; ++r) {
        rows[r].qkv = d_qkv + (size_t)r * t->ldqkv;
        rows[r].out = d_out + (size_t)r * H * hd;
        rows[r].kc = d_k + (size_t)t->slot[r] * cache_n;
        rows[r].vc = d_v + (size_t)t->slot[r] * cache_n;
        rows[r].rope = d_rope + r * rw;
        rows[r].pos = d_pos + r;
    }
    GHIP_CHECK(hipMemcpy(d_rows, rows.data(), (size_t)Rn * sizeof(slot_row), hipMemcpyHostToDevice));
    attn_args a{};
    a.rope_cos = d_c; a.rope_sin = d_s;
    a.H = H; a.Hkv = Hkv; a.hd = hd; a.ctx = ctx; a.q_scale = t->q_scale;
    a.mode = ATTN_SPLIT;
    const int r = launch_attn_long_rows(a, d_rows, R, 0, d_sb, d_pb, nullptr);
    GHIP_CHECK(hipDeviceSynchronize());
    if (r != 0) return r;
    GHIP_CHECK(hipMemcpy(t->out, d_out, out_n * 4, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(t->kc, d_k, (size_t)t->n_slots * cache_n * 2, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(t->vc, d_v, (size_t)t->n_slots * cache_n * 2, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(sb.data(), d_sb, tap_n * 4, hipMemcpyDeviceToHost));
    GHIP_CHECK(hipMemcpy(t->dbg_p, d_pb, tap_n * 2, hipMemcpyDeviceToHost));  // [R][H][ctx] as it is
    for (int rr = 0; rr < Rn; ++rr)  // the scores [R][Hkv][ctx][G] by head
        for (int h = 0; h < H; ++h)
            for (int j = 0; j < ctx; ++j)
                t->dbg_w[((size_t)rr * H + h) * ctx + j] = sb[(((size_t)rr * Hkv + h / G) * ctx + j) * G + h % G];
    return 0;
}

extern "C" int gemma_test_exp_f16(uint16_t *out) {
    set_error("");
    dev_pool tmp;
    uint16_t *d = nullptr;
    if (tmp.get(&d, 65536 * 2)) return -1;
    int r = launch_exp_f16_all(d, nullptr);
    if (r == 0) GHIP_CHECK(hipMemcpy(out, d, 65536 * 2, hipMemcpyDeviceToHost));
    return r;
}

// Test hook: one rms_norm kernel on `rows` host rows of n f32.  kind 0: the ggml
// executor's RMS_NORM (k_g_rms_norm), out = f32 rows x * scale; kind 1: k_norm_q8K (rms_norm * w then
// quantize_row_q8_K, n a multiple of 256, <= 4096), out = Q8_K rows.
extern "C" int gemma_test_rms_norm(int kind, const float *x, const float *w, int rows, int n, float eps, void *out) {
    set_error("");
    if (rows <= 0 || n <= 0 || (kind == 1 && (n % 256 || n > 4096)) || kind < 0 || kind > 1) {
        set_error("gemma_test_rms_norm: unsupported shape or kind");
        return -1;
    }
    const size_t in_b = (size_t)rows * n * 4, out_b = kind == 0 ? in_b : (size_t)rows * (n / 256) * 292;
    float *dx = nullptr, *dw = nullptr;
    uint8_t *dy = nullptr;
    dev_pool tmp;
    if (tmp.get(&dx, in_b) || tmp.get(&dw, (size_t)n * 4) || tmp.get(&dy, out_b)) return -1;
    GHIP_CHECK(hipMemcpy(dx, x, in_b, hipMemcpyHostToDevice));
    if (w) GHIP_CHECK(hipMemcpy(dw, w, (size_t)n * 4, hipMemcpyHostToDevice));
    int r;
    if (kind == 0) {
        gt_desc a, d;
        a.data = (char *)dx;
        d.data = (char *)dy;
        a.ne[0] = d.ne[0] = n;
        a.ne[1] = d.ne[1] = rows;
        a.nb[0] = d.nb[0] = 4;
        a.nb[1] = d.nb[1] = (int64_t)n * 4;
        a.nb[2] = d.nb[2] = a.nb[3] = d.nb[3] = (int64_t)n * rows * 4;
        r = launch_g_rms_norm(a, d, eps, nullptr);
    } else {
        r = launch_norm_q8K(dx, n, dw, n, eps, rows, dy, (n / 256) * 292, nullptr);
    }
    if (r == 0) GHIP_CHECK(hipMemcpy(out, dy, out_b, hipMemcpyDeviceToHost));
    return r;
}

// Measured HBM read roofline: a streaming read of `bytes` (>= 4 GB defeats the
// Infinity Cache), `iters` passes timed with hipEvents; returns GB/s (negative on error).
// measured HBM read rate (GB/s) of one probe: variant 0 = 16-B nontemporal loads into VGPRs (8 in
// flight per lane), 1 = LDS-DMA (global_load_lds_dwordx4 nt, 16 KiB in flight per wave); a buffer
// far beyond the 256 MB Infinity Cache
extern "C" double gemma_hbm_read_probe(int device, size_t bytes, int iters, int variant) {
    set_error("");
    if (hipSetDevice(device) != hipSuccess) return -1.0;
    void *buf = nullptr;
    unsigned *sink = nullptr;
    dev_pool tmp;
    if (tmp.get(&buf, bytes) || tmp.get(&sink, 4)) return -1.0;
    (void)hipMemset(buf, 1, bytes);
    hipStream_t s;
    (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    double gbs = -1.0;
    if (launch_stream_read(buf, bytes, sink, s, variant) == 0) {
        (void)hipEventRecord(t0, s);
        for (int i = 0; i < iters; ++i) (void)launch_stream_read(buf, bytes, sink, s, variant);
        (void)hipEventRecord(t1, s);
        (void)hipEventSynchronize(t1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, t0, t1);
        gbs = (double)bytes * iters / (ms * 1e-3) / 1e9;
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipStreamDestroy(s);
    return gbs;
}

// the measured HBM read roofline: the faster of the two probes
extern "C" double gemma_hbm_read_gbs(int device, size_t bytes, int iters) {
    const double a = gemma_hbm_read_probe(device, bytes, iters, 0), b = gemma_hbm_read_probe(device, bytes, iters, 1);
    return a > b ? a : b;
}
