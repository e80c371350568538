"""What the picks of a batched-decode pass cost with a sampler per slot: Gemma-2B Q4_0 (synthetic
weights, the BASELINE config 2 shape), n_ctx 512, one engine, one process.

    python scripts/batch_sampler_bench.py [--reps 3] [--prompt 128] [--iters 24] [--R 8,64]
                                          [--legs engine_k40,slots_k40,mixed,slots_greedy,engine_greedy]
                                          [--out FILE]

Every slot is adopted from its own `prompt`-token prefilled prompt; a leg is 8 warm-up passes, then
`iters` passes in ONE gemma_engine_batch_step call (one host sync).  Legs, alternated `reps` times at
each R:
    engine_k40     the engine's sampler, T 0.8 / top_k 40 / top_p 0.95, no slot setting (3 pick launches)
    slots_k40      every slot those parameters as its own, a seed per slot              (3)
    mixed          even slots their own greedy, odd slots k40                           (4)
    slots_greedy   the engine's sampler on, every slot its own greedy                   (1)
    engine_greedy  no sampler anywhere                                                  (1)
A library without gemma_engine_batch_set_sampler (an older build, for an A/B) runs the two engine legs.
Prints one line per timed leg and a JSON summary: per leg and R the median with min - max over the
alternations, in µs per pass."""
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
K40 = dict(temperature=0.8, top_k=40, top_p=0.95)
LEGS = ["engine_k40", "slots_k40", "mixed", "slots_greedy", "engine_greedy"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--R", default="8,64")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    args = ap.parse_args()
    Rs = [int(t) for t in args.R.split(",")]
    per_slot = hasattr(G.Engine, "batch_set_sampler")
    legs = [leg for leg in args.legs.split(",") if per_slot or leg.startswith("engine_")]
    assert all(leg in LEGS for leg in legs), legs
    e = G.Engine(GEMMA_2B, n_ctx=args.ctx)
    n_max = max(Rs)
    prompts = [[int(t) for t in make_prompt(args.prompt, GEMMA_2B["n_vocab"], seed=1 + s)] for s in range(n_max)]

    def settings(leg, R):
        """the engine's sampler and the slots' own for this leg"""
        if leg in ("engine_k40", "slots_greedy"):
            e.set_sampler(seed=1, **K40)
        else:
            e.set_sampler(None)
        if not per_slot:
            return
        for s in range(R):
            if leg == "slots_k40" or (leg == "mixed" and s % 2 == 1):
                e.batch_set_sampler(s, seed=100 + s, **K40)
            elif leg == "slots_greedy" or leg == "mixed":
                e.batch_set_sampler(s, temperature=0.0)
            else:
                e.batch_set_sampler(s)

    res = {}
    for R in Rs:
        if R <= G.BATCH_MAX_SLOTS:
            e.batch_open(R)
        else:
            e.batch_open_wide(R)
        for rep in range(args.reps):
            for leg in legs:
                settings("engine_greedy", R)  # every slot's pending token by the same (greedy) prefill pick
                for s in range(R):
                    e.begin(prompts[s])
                    e.prefill(args.prompt)
                    e.batch_adopt(s)
                settings(leg, R)
                e.batch_step(WARM)
                t0 = time.perf_counter()
                e.batch_step(args.iters)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                assert all(e.batch_pos(s) == args.prompt + WARM + args.iters for s in range(R))
                res.setdefault(f"{leg}@{R}", []).append(us)
                print(f"rep {rep} R={R:2d} {leg:13s} {us:9.1f} us/pass  {us / R:8.1f} us/token", flush=True)
        e.batch_close()
    out = {}
    for k, v in res.items():
        v = sorted(v)
        out[k] = dict(us_median=round(v[len(v) // 2], 1), us_min=round(v[0], 1), us_max=round(v[-1], 1),
                      spread_us=round(v[-1] - v[0], 1))
    line = json.dumps(dict(prompt=args.prompt, iters=args.iters, reps=args.reps, ctx=args.ctx, per_slot=per_slot, legs=out))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
