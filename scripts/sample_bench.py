"""What on-device sampling costs: Gemma-2B Q4_0 (synthetic weights, the BASELINE config 2 shape),
one engine, one process.

    python scripts/sample_bench.py [--steps 512] [--reps 3] [--prompt 128] [--legs greedy,k40,k1024,host]

Legs, alternated `reps` times, each from the same state (begin, the prompt and 8 warm-up steps by
graph replay, then `steps` timed graph replays with no host sync in between):
    greedy   the default: k_advance on the logits launch's argmax keys
    k40      set_sampler(T = 0.8, top_k = 40, top_p = 0.95)
    k1024    set_sampler(T = 0.8, top_k = 1024, top_p = 1)
    host     the only way to sample without the feature: step(1, want_logits) per token, a numpy draw
             on the host (T = 0.8, top_k = 40, top_p = 0.95), the token fed back through extend()
Prints one line per timed leg and a JSON summary (tok/s median and spread, launches per token).
Under `rocprofv3 --kernel-trace --stats` run one short sampled leg (--legs k40 --reps 1 --steps 64):
the k_sample_* rows of the kernel stats are the sampler's own time."""
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

SAMPLERS = {"greedy": None, "k40": dict(temperature=0.8, top_k=40, top_p=0.95, seed=1),
            "k1024": dict(temperature=0.8, top_k=1024, top_p=1.0, seed=1)}


def host_draw(row, rng, temperature=0.8, top_k=40, top_p=0.95):
    """a plain numpy top-k / top-p draw (timing contrast only; not the engine's seeded rule)"""
    idx = np.argpartition(row, -top_k)[-top_k:]
    idx = idx[np.argsort(-row[idx], kind="stable")]
    w = np.exp((row[idx].astype(np.float64) - float(row[idx[0]])) / temperature)
    c = np.cumsum(w)
    m = int(np.searchsorted(c, top_p * c[-1], side="left")) + 1
    return int(idx[min(int(np.searchsorted(c[:m], rng.random() * c[m - 1], side="right")), m - 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--legs", default="greedy,k40,k1024,host")
    ap.add_argument("--no-tune", action="store_true")
    args = ap.parse_args()
    legs = args.legs.split(",")
    n_ctx = ((args.prompt + args.warmup + args.steps + 64) // 32 + 1) * 32
    e = G.Engine(GEMMA_2B, n_ctx=n_ctx)
    if not args.no_tune:
        e.tune(8)
    prompt = make_prompt(args.prompt, GEMMA_2B["n_vocab"])
    res = {k: [] for k in legs}
    launches = {}
    for rep in range(args.reps):
        for leg in legs:
            if leg == "host":
                e.set_sampler(None)
            else:
                e.set_sampler(**SAMPLERS[leg]) if SAMPLERS[leg] else e.set_sampler(None)
            e.begin(prompt)
            e.step(args.prompt + args.warmup, use_graph=True)
            e.sync()
            t0 = time.perf_counter()
            if leg == "host":
                rng = np.random.default_rng(1)
                for _ in range(args.steps):
                    lg = e.step(1, want_logits=True, use_graph=True)
                    e.extend([host_draw(lg[0], rng)], keep=e.pos())
            else:
                e.step(args.steps, use_graph=True)
            e.sync()
            dt = time.perf_counter() - t0
            res[leg].append(args.steps / dt)
            launches[leg] = e.graph_kernels()
            print(f"rep {rep} {leg:7s} {args.steps / dt:8.1f} tok/s  {dt / args.steps * 1e6:7.1f} us/token  "
                  f"launches/token {launches[leg]}  tail {list(e.tokens()[-4:])}", flush=True)
    out = {}
    for leg in legs:
        v = sorted(res[leg])
        out[leg] = dict(tok_s_median=round(v[len(v) // 2], 1), tok_s_min=round(v[0], 1), tok_s_max=round(v[-1], 1),
                        us_per_token_median=round(1e6 / v[len(v) // 2], 1), launches_per_token=launches[leg])
    print(json.dumps(dict(steps=args.steps, reps=args.reps, prompt=args.prompt, legs=out)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
