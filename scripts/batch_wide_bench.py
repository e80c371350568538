"""What a wide batched-decode pass costs in its two forms: Gemma-2B Q4_0 (synthetic weights, the
BASELINE config 2 shape), n_ctx 512, one engine, one process, in the manner of scripts/batch_bench.py.

    python scripts/batch_wide_bench.py [--reps 3] [--prompt 128] [--iters 24]
                                       [--R 8,9,12,16,24,32,48,64] [--forms mfma,groups] [--out FILE]

A leg is (R, form): every one of the R slots adopted from its own `prompt`-token prefilled prompt, 8
warm-up passes, then `iters` passes in ONE gemma_engine_batch_step call (one host sync).  form mfma sets
bt_mfma_min = 9 (one pass on the exact MFMA GEMMs), groups sets 65 (groups of up to 8 rows on the
skinny GEMM); R <= 8 is the skinny pass in either.  The legs are alternated `reps` times.
Prints one line per timed leg and a JSON summary: medians with min - max, aggregate tok/s = R / t, and
the smallest R from which the MFMA form is faster at every larger R measured (the default of
bt_mfma_min).  Under `rocprofv3 --kernel-trace --stats` run one leg alone (--R 64 --forms mfma
--reps 1): the process launches eagerly only (no tune, no graph replay)."""
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
FORMS = dict(mfma=9, groups=G.BATCH_WIDE_MAX_SLOTS + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--R", default="8,9,12,16,24,32,48,64")
    ap.add_argument("--forms", default="mfma,groups")
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    args = ap.parse_args()
    Rs = [int(t) for t in args.R.split(",")]
    forms = args.forms.split(",")
    NS = max(Rs)
    e = G.Engine(GEMMA_2B, n_ctx=args.ctx)
    prompts = [[int(t) for t in make_prompt(args.prompt, GEMMA_2B["n_vocab"], seed=1 + s)] for s in range(NS)]
    e.batch_open_wide(NS)
    res = {}
    for rep in range(args.reps):
        for R in Rs:
            for form in forms:
                e.set_option("bt_mfma_min", FORMS[form])
                for s in range(NS):
                    e.batch_release(s)
                for s in range(R):
                    e.begin(prompts[s])
                    e.prefill(args.prompt)
                    e.batch_adopt(s)
                e.batch_step(WARM)
                t0 = time.perf_counter()
                e.batch_step(args.iters)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                res.setdefault((R, form), []).append(us)
                assert all(e.batch_pos(s) == args.prompt + WARM + args.iters for s in range(R))
                print(f"rep {rep} R={R:2d} {form:6s} {us:9.1f} us/pass  {us / R:7.1f} us/token  {R / us * 1e6:9.1f} tok/s", flush=True)
    legs = {}
    for (R, form), v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        legs[f"R{R}_{form}"] = dict(us_median=round(med, 1), us_min=round(v[0], 1), us_max=round(v[-1], 1),
                                    tok_s_aggregate=round(R / med * 1e6, 1), tok_s_min=round(R / v[-1] * 1e6, 1),
                                    tok_s_max=round(R / v[0] * 1e6, 1))
    summary = {}
    if set(forms) == {"mfma", "groups"}:
        wide = [R for R in sorted(Rs) if R > G.BATCH_MAX_SLOTS]
        faster = {R: legs[f"R{R}_mfma"]["us_median"] < legs[f"R{R}_groups"]["us_median"] for R in wide}
        best = G.BATCH_WIDE_MAX_SLOTS + 1
        for R in reversed(wide):
            if not faster[R]:
                break
            best = R
        summary["bt_mfma_min_measured"] = best
    line = json.dumps(dict(prompt=args.prompt, iters=args.iters, reps=args.reps, ctx=args.ctx, legs=legs, **summary))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
