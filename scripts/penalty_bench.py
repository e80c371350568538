"""What the penalties cost: Gemma-2B Q4_0 (synthetic weights, the BASELINE config 2 shape), one engine,
one process, the set-up of scripts/sample_bench.py.

    python scripts/penalty_bench.py [--steps 256] [--reps 3] [--prompt 128] [--ctx 0] [--legs greedy,greedy+64,k40,k40+64]

A leg is a sampler (greedy, k40: T = 0.8, top_k = 40, top_p = 0.95) and, behind a `+`, the last_n of
set_penalties(repeat 1.1, presence 0, frequency 0); no `+`: penalties off.  Legs are alternated `reps`
times, each from the same state: the sequence rewound to the end of the prompt (extend), 8 warm-up graph
replays, then `steps` timed replays with no host sync in between.  --ctx 8192 --prompt 7900 puts the timed
steps at positions whose window of last_n 8192 fills the 8,192-entry sort.  The prompt is consumed once,
by decode steps.  Prints one line per timed leg and a JSON summary (tok/s median and spread, launches per
token).  Under `rocprofv3 --kernel-trace --stats` run one short leg per setting (--reps 1 --steps 64): the
k_penalty_apply / k_penalty_restore rows of the kernel stats are the feature's own time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: the HIP runtime the tests and bench.py run on)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, ROOT)

import gemma_hip as G  # noqa: E402
from bench import GEMMA_2B, make_prompt  # noqa: E402

K40 = dict(temperature=0.8, top_k=40, top_p=0.95, seed=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=0, help="n_ctx (0: just enough for the prompt and the steps)")
    ap.add_argument("--legs", default="greedy,greedy+64,k40,k40+64")
    ap.add_argument("--op", type=int, default=0, help="instead: 32 calls of the two kernels alone on one 256,000-logit row "
                    "with a window of this many random tokens (gemma_test_penalize; for a kernel trace)")
    args = ap.parse_args()
    if args.op:
        rng = np.random.default_rng(1)
        V = GEMMA_2B["n_vocab"]
        row = rng.standard_normal((1, V)).astype(np.float32)
        for _ in range(32):
            hist = rng.integers(0, V, (1, args.op)).astype(np.int32)
            _, _, n_saved = G.test_penalize(row, hist, [args.op - 1], (1.1, 0.0, 0.0, args.op))
        print(f"op: window {args.op}, {int(n_saved[0])} distinct tokens in the last call", flush=True)
        return
    legs = args.legs.split(",")
    n_ctx = args.ctx or ((args.prompt + args.warmup + args.steps + 64) // 32 + 1) * 32
    e = G.Engine(GEMMA_2B, n_ctx=n_ctx)
    e.tune(8)
    prompt = make_prompt(args.prompt, GEMMA_2B["n_vocab"])
    e.begin(prompt)
    e.step(args.prompt - 1, use_graph=True)  # the prompt once; every leg rewinds to its last token
    res, launches = {k: [] for k in legs}, {}
    for rep in range(args.reps):
        for leg in legs:
            smp, _, last_n = leg.partition("+")
            e.set_sampler(**K40) if smp == "k40" else e.set_sampler(None)
            e.set_penalties(1.1, 0.0, 0.0, int(last_n)) if last_n else e.set_penalties(None)
            e.extend([int(prompt[-1])], keep=args.prompt - 1)
            e.step(args.warmup, use_graph=True)
            e.sync()
            t0 = time.perf_counter()
            e.step(args.steps, use_graph=True)
            e.sync()
            dt = time.perf_counter() - t0
            res[leg].append(args.steps / dt)
            launches[leg] = e.graph_kernels()
            print(f"rep {rep} {leg:12s} {args.steps / dt:8.1f} tok/s  {dt / args.steps * 1e6:7.1f} us/token  "
                  f"launches/token {launches[leg]}  pos {e.pos()}  tail {list(e.tokens()[-4:])}", flush=True)
    out = {}
    for leg in legs:
        v = sorted(res[leg])
        out[leg] = dict(tok_s_median=round(v[len(v) // 2], 1), tok_s_min=round(v[0], 1), tok_s_max=round(v[-1], 1),
                        us_per_token_median=round(1e6 / v[len(v) // 2], 1), launches_per_token=launches[leg])
    print(json.dumps(dict(steps=args.steps, reps=args.reps, prompt=args.prompt, n_ctx=n_ctx, legs=out)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
