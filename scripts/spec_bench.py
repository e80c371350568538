"""What a speculative verify pass costs beside plain decode steps: Gemma-2B Q4_0 (synthetic weights,
the BASELINE config 2 shape), one engine, one process.

    python scripts/spec_bench.py [--reps 3] [--prompt 128] [--iters 24] [--T 2,4,8] [--out FILE]

Legs, alternated `reps` times, each from the same state (the prompt by the exact batched prefill, 8
warm-up graph steps):
    step        t_step: `iters` x 8 graph replays, no host sync in between
    verify T    t_verify(T): `iters` gemma_engine_verify calls of k = T - 1 drafts taken from a prior
                plain run, so every draft is accepted and a pass appends T tokens
    x4 T        the same pass through the path without the feature: extend(keep = pos, [pending token,
                drafts]) + prefill_next(T, logits_all) on the exact prefill GEMM (k_gemm_x4); the host
                round trips it needs (rows copied out) are part of its time
Prints one line per timed leg and a JSON summary: medians with min - max, the break-even accepted
drafts per pass t_verify(T) / t_step - 1, and the tok/s at full acceptance T / t_verify(T).
Under `rocprofv3 --kernel-trace --stats` run one short leg (--reps 1 --iters 4 --T 8 --legs verify):
the k_gemm_skinny rows are the GEMM's own time per matrix class."""
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
    ap.add_argument("--T", default="2,4,8")
    ap.add_argument("--legs", default="step,verify,x4")
    ap.add_argument("--no-tune", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    args = ap.parse_args()
    Ts = [int(t) for t in args.T.split(",")]
    legs = args.legs.split(",")
    span = args.iters * 8
    n_ctx = ((args.prompt + WARM + span + 64) // 32 + 1) * 32
    e = G.Engine(GEMMA_2B, n_ctx=n_ctx)
    if not args.no_tune:
        e.tune(8)
    prompt = [int(t) for t in make_prompt(args.prompt, GEMMA_2B["n_vocab"])]

    def start():
        e.begin(prompt)
        e.prefill(len(prompt))
        e.step(WARM, use_graph=True)
        e.sync()

    start()
    e.step(span + 8, use_graph=True)
    ref = [int(t) for t in e.tokens()]  # the plain run the drafts are taken from
    res = {}
    for rep in range(args.reps):
        if "step" in legs:
            start()
            t0 = time.perf_counter()
            e.step(span, use_graph=True)
            e.sync()
            us = (time.perf_counter() - t0) / span * 1e6
            res.setdefault("step", []).append(us)
            print(f"rep {rep} step        {us:8.1f} us/token  launches/token {e.graph_kernels()}", flush=True)
        for T in Ts:
            if "verify" in legs:
                start()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    pos = e.pos()
                    got = e.verify(ref[pos + 1:pos + T])
                    assert len(got) == T, (T, got, ref[pos + 1:pos + T + 1])
                us = (time.perf_counter() - t0) / args.iters * 1e6
                res.setdefault(f"verify{T}", []).append(us)
                assert [int(t) for t in e.tokens()] == ref[:e.pos() + 1]
                print(f"rep {rep} verify T={T}  {us:8.1f} us/pass   {us / T:7.1f} us/token", flush=True)
            if "x4" in legs:
                start()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    pos = e.pos()
                    e.extend(ref[pos:pos + T], keep=pos)
                    e.prefill_next(T, want_all=True)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                res.setdefault(f"x4_{T}", []).append(us)
                print(f"rep {rep} x4     T={T}  {us:8.1f} us/pass   {us / T:7.1f} us/token", flush=True)
    out = {}
    for k, v in res.items():
        v = sorted(v)
        out[k] = dict(us_median=round(v[len(v) // 2], 1), us_min=round(v[0], 1), us_max=round(v[-1], 1))
    if "step" in out:
        ts = out["step"]["us_median"]
        for T in Ts:
            if f"verify{T}" in out:
                tv = out[f"verify{T}"]["us_median"]
                out[f"verify{T}"].update(break_even_accepted=round(tv / ts - 1, 2), tok_s_full_accept=round(T / tv * 1e6, 1),
                                         worth_having=bool(tv < T * ts))
        out["step"]["tok_s"] = round(1e6 / ts, 1)
    line = json.dumps(dict(prompt=args.prompt, iters=args.iters, reps=args.reps, legs=out))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
