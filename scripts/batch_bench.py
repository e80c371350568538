"""What a batched-decode pass costs beside single-sequence steps and beside the verify pass with the
same GEMMs: Gemma-2B Q4_0 (synthetic weights, the BASELINE config 2 shape), n_ctx 512, one engine, one
process.

    python scripts/batch_bench.py [--reps 3] [--prompt 128] [--iters 24] [--R 1,2,4,8]
                                  [--legs step,batch,verify] [--out FILE]

Legs, alternated `reps` times:
    step        t_step: `iters` graph replays of the engine's own sequence (prompt by the exact batched
                prefill, 8 warm-up steps), no host sync in between: the single-stream baseline
    batch R     t_batch(R): every slot adopted from its own `prompt`-token prefilled prompt, 8 warm-up
                passes, then `iters` passes in ONE gemma_engine_batch_step call (one host sync)
    verify T    t_verify(T) for T = R >= 2: `iters` gemma_engine_verify calls of k = T - 1 drafts taken
                from a prior plain run (all accepted): the pass with the same GEMMs and the
                single-sequence attention; each call ends with its own host sync
Prints one line per timed leg and a JSON summary: medians with min - max, aggregate tok/s =
R / t_batch(R), whether R passes beat R single steps, and the smallest R at which they do.
Under `rocprofv3 --kernel-trace --stats` run the batch leg alone (--legs batch --R 8 --reps 1): that
process launches eagerly only (no tune, no graph replay)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime the tests and bench.py run on)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, ROOT)

import gemma_hip as G  # noqa: E402
from bench import GEMMA_2B, make_prompt  # noqa: E402

WARM = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--R", default="1,2,4,8")
    ap.add_argument("--legs", default="step,batch,verify")
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    args = ap.parse_args()
    Rs = [int(t) for t in args.R.split(",")]
    legs = args.legs.split(",")
    graphs = "step" in legs or "verify" in legs  # the batch leg alone stays eager: no tune, no replay
    e = G.Engine(GEMMA_2B, n_ctx=args.ctx)
    if graphs:
        e.tune(8)
    prompts = [[int(t) for t in make_prompt(args.prompt, GEMMA_2B["n_vocab"], seed=1 + s)] for s in range(G.BATCH_MAX_SLOTS)]

    def start():
        e.begin(prompts[0])
        e.prefill(args.prompt)
        e.step(WARM, use_graph=True)
        e.sync()

    ref = None
    if "verify" in legs:
        start()
        e.step(args.iters * max(Rs) + 8, use_graph=True)
        ref = [int(t) for t in e.tokens()]  # the plain run the drafts are taken from
    e.batch_open(G.BATCH_MAX_SLOTS)
    res = {}
    for rep in range(args.reps):
        if "step" in legs:
            start()
            t0 = time.perf_counter()
            e.step(args.iters, use_graph=True)
            e.sync()
            us = (time.perf_counter() - t0) / args.iters * 1e6
            res.setdefault("step", []).append(us)
            print(f"rep {rep} step        {us:8.1f} us/token  launches/token {e.graph_kernels()}", flush=True)
        for R in Rs:
            if "batch" in legs:
                for s in range(G.BATCH_MAX_SLOTS):
                    e.batch_release(s)
                for s in range(R):
                    e.begin(prompts[s])
                    e.prefill(args.prompt)
                    e.batch_adopt(s)
                e.batch_step(WARM)
                t0 = time.perf_counter()
                e.batch_step(args.iters)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                res.setdefault(f"batch{R}", []).append(us)
                assert all(e.batch_pos(s) == args.prompt + WARM + args.iters for s in range(R))
                print(f"rep {rep} batch  R={R}  {us:8.1f} us/pass   {us / R:7.1f} us/token", flush=True)
            if "verify" in legs and R >= 2:
                start()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    pos = e.pos()
                    got = e.verify(ref[pos + 1:pos + R])
                    assert len(got) == R, (R, got)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                res.setdefault(f"verify{R}", []).append(us)
                print(f"rep {rep} verify T={R}  {us:8.1f} us/pass   {us / R:7.1f} us/token", flush=True)
    out = {}
    for k, v in res.items():
        v = sorted(v)
        out[k] = dict(us_median=round(v[len(v) // 2], 1), us_min=round(v[0], 1), us_max=round(v[-1], 1))
    summary = {}
    if "step" in out:
        ts = out["step"]["us_median"]
        spread = round(out["step"]["us_max"] - out["step"]["us_min"], 1)
        out["step"].update(tok_s=round(1e6 / ts, 1), spread_us=spread)
        pays = []
        for R in Rs:
            if f"batch{R}" not in out:
                continue
            tb = out[f"batch{R}"]["us_median"]
            out[f"batch{R}"].update(tok_s_aggregate=round(R / tb * 1e6, 1), beats_R_single_steps=bool(tb < R * ts))
            if tb < R * ts:
                pays.append(R)
            if f"verify{R}" in out:
                out[f"batch{R}"]["us_over_verify"] = round(tb - out[f"verify{R}"]["us_median"], 1)
        summary["smallest_R_that_pays"] = min(pays) if pays else None
    line = json.dumps(dict(prompt=args.prompt, iters=args.iters, reps=args.reps, ctx=args.ctx, legs=out, **summary))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
