"""What a batch pass with per-slot drafts costs (gemma_engine_batch_verify) beside the one-row batch
pass and beside a step_rows pass of the same row count: Gemma-2B Q4_0 (synthetic weights, the BASELINE
config 2 shape), n_ctx 512, slots adopted from 128-token prompts, one engine, one process (the set-up of
scripts/batch_bench.py).

    python scripts/batch_spec_bench.py [--reps 3] [--iters 24] [--R 1,2,4,8] [--k 3,7]
                                       [--legs batch,rows,bverify] [--tree DIR] [--out FILE]
    python scripts/batch_spec_bench.py --summarize NEW.json ... [--parent PARENT.json ...] [--out FILE]

Legs, alternated `reps` times:
    batch R       t_batch(R): R slots, 8 warm-up passes, `iters` passes in ONE gemma_engine_batch_step
                  call (one host sync)
    rows R,k      a gemma_engine_batch_step_rows pass of the same T = R * (1 + k) rows: slot 0 still has
                  given tokens to consume and takes 1 + R * k rows, slots 1 .. R-1 decode one row each;
                  as many passes as fit n_ctx, `iters` at most, each call with its own host sync
    bverify R,k   t_bverify(R, k): `iters` gemma_engine_batch_verify calls, every slot with k drafts taken
                  from a prior plain run (all accepted, checked), each call with its own host sync
--tree DIR runs another checkout's binding and library (an A/B leg of another build, e.g. the parent
commit's: it has the batch and rows legs only).  --summarize folds the JSON files of several runs:
medians with min - max per leg, per (R, k) the difference to the parent's step_rows pass of the same T,
the break-even accepted drafts per slot and pass t_bverify / t_batch(R) - 1, the aggregate tok/s at
full acceptance R * (1 + k) / t_bverify, and the one condition: at R = 2, k = 3 the minimum of this
build's aggregate tok/s over the repetitions lies above the maximum of the parent's batch_step at R = 2.
Under `rocprofv3 --kernel-trace --stats` run one leg alone (--legs bverify --R 2 --k 3 --reps 1)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime the tests and bench.py run on)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 8
PROMPT = 128


def _stats(v):
    v = sorted(v)
    return dict(us_median=round(v[len(v) // 2], 1), us_min=round(v[0], 1), us_max=round(v[-1], 1))


def summarize(new_files, parent_files, out_file):
    def fold(files):
        raw = {}
        for f in files:
            for leg, v in json.loads(open(f).read().strip().splitlines()[-1])["raw"].items():
                raw.setdefault(leg, []).extend(v)
        return raw

    new, par = fold(new_files), fold(parent_files)
    legs = {k: _stats(v) for k, v in new.items()}
    parent = {k: _stats(v) for k, v in par.items()}
    table = []
    for leg in sorted(k for k in new if k.startswith("bverify")):
        R, k = (int(t) for t in leg[len("bverify"):].split("_"))
        tv, tb = legs[leg]["us_median"], legs[f"batch{R}"]["us_median"]
        row = dict(R=R, k=k, T=R * (1 + k), t_bverify_us=tv, t_batch_us=tb, break_even_accepted=round(tv / tb - 1, 2),
                   tok_s_full_acceptance=round(R * (1 + k) / tv * 1e6, 1))
        if f"rows{R}_{k}" in legs:
            row["over_rows_us"] = round(tv - legs[f"rows{R}_{k}"]["us_median"], 1)
        if f"rows{R}_{k}" in parent:
            row["over_parent_rows_us"] = round(tv - parent[f"rows{R}_{k}"]["us_median"], 1)
        table.append(row)
    res = dict(legs=legs, parent=parent, table=table)
    if "bverify2_3" in new and "batch2" in par:
        lo = min(2 * 4 / t * 1e6 for t in new["bverify2_3"])
        hi = max(2 / t * 1e6 for t in par["batch2"])
        res["condition_R2_k3"] = dict(min_tok_s_this_build=round(lo, 1), max_tok_s_parent_batch_step=round(hi, 1),
                                      holds=bool(lo > hi), ratio=round(lo / hi, 2))
    line = json.dumps(res)
    print(line, flush=True)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--R", default="1,2,4,8")
    ap.add_argument("--k", default="3,7")
    ap.add_argument("--legs", default="batch,rows,bverify")
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose binding and library run")
    ap.add_argument("--summarize", nargs="+", default=None, metavar="JSON", help="fold these runs' files instead of running")
    ap.add_argument("--parent", nargs="+", default=[], metavar="JSON", help="with --summarize: the parent build's runs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.parent, args.out)
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "gemma.ggml_amd", "python"))
    sys.path.insert(0, ROOT)
    import numpy as np
    import gemma_hip as G
    from bench import GEMMA_2B, make_prompt

    Rs, ks, legs = [int(t) for t in args.R.split(",")], [int(t) for t in args.k.split(",")], args.legs.split(",")
    NS, KD, V = G.BATCH_MAX_SLOTS, G.VERIFY_MAX_DRAFT, GEMMA_2B["n_vocab"]
    e = G.Engine(GEMMA_2B, n_ctx=args.ctx)
    prompts = [[int(t) for t in make_prompt(PROMPT, V, seed=1 + s)] for s in range(NS)]
    long0 = [int(t) for t in make_prompt(args.ctx - 1, V, seed=1)]  # slot 0 of the rows leg: given tokens to consume
    e.batch_open_rows(NS, G.BATCH_WIDE_MAX_SLOTS)

    def adopt(R, first_long=False):
        for s in range(NS):
            e.batch_release(s)
        for s in range(R):
            e.begin(long0 if (first_long and s == 0) else prompts[s])
            if first_long and s == 0:
                e.prefill_next(PROMPT)
            else:
                e.prefill(PROMPT)
            e.batch_adopt(s)

    refs = None
    if "bverify" in legs:  # the plain run the drafts are taken from
        adopt(max(Rs))
        e.batch_step(WARM + args.iters * (1 + max(ks)) + KD + 1)
        refs = [[int(t) for t in e.batch_tokens(s)] for s in range(max(Rs))]
    raw = {}
    for rep in range(args.reps):
        for R in Rs:
            if "batch" in legs:
                adopt(R)
                e.batch_step(WARM)
                t0 = time.perf_counter()
                e.batch_step(args.iters)
                us = (time.perf_counter() - t0) / args.iters * 1e6
                raw.setdefault(f"batch{R}", []).append(us)
                print(f"rep {rep} batch   R={R}      {us:8.1f} us/pass  {R / us * 1e6:8.1f} tok/s", flush=True)
            for k in ks:
                T = R * (1 + k)
                if "rows" in legs:
                    adopt(R, first_long=True)
                    e.batch_step(WARM)
                    n = min(args.iters, (args.ctx - 2 - PROMPT - WARM) // (1 + R * k))
                    t0 = time.perf_counter()
                    for _ in range(n):
                        rows_of, _lg = e.batch_step_rows(T)
                    us = (time.perf_counter() - t0) / n * 1e6
                    assert int(rows_of.sum()) == T and rows_of[0] == 1 + R * k, list(rows_of)
                    raw.setdefault(f"rows{R}_{k}", []).append(us)
                    print(f"rep {rep} rows    R={R} k={k}  {us:8.1f} us/pass  T={T} ({n} passes)", flush=True)
                if "bverify" in legs:
                    adopt(R)
                    e.batch_step(WARM)
                    calls = []
                    for i in range(args.iters):  # every pass's arguments, made before the clock starts
                        pos = PROMPT + WARM + i * (1 + k)
                        d = np.zeros((NS, KD), dtype=np.int32)
                        for s in range(R):
                            d[s, :k] = refs[s][pos + 1:pos + 1 + k]
                        k_of = np.full(NS, k, dtype=np.int32)
                        calls.append((d, k_of, np.zeros((NS, KD + 1), dtype=np.int32), np.zeros(NS, dtype=np.int32)))
                    t0 = time.perf_counter()
                    for d, k_of, out, n_out in calls:
                        e.L.gemma_engine_batch_verify(e.h, G._p(d), G._p(k_of), G._p(out), G._p(n_out), None)
                    us = (time.perf_counter() - t0) / args.iters * 1e6
                    assert all((c[3][:R] == k + 1).all() for c in calls), "a draft of the plain run was rejected"
                    assert all(e.batch_pos(s) == PROMPT + WARM + args.iters * (1 + k) for s in range(R))
                    raw.setdefault(f"bverify{R}_{k}", []).append(us)
                    print(f"rep {rep} bverify R={R} k={k}  {us:8.1f} us/pass  T={T}  {T / us * 1e6:8.1f} tok/s at full acceptance",
                          flush=True)
    line = json.dumps(dict(tree=os.path.relpath(os.path.abspath(args.tree), ROOT), prompt=PROMPT, iters=args.iters, reps=args.reps, ctx=args.ctx,
                           legs={k: _stats(v) for k, v in raw.items()}, raw=raw))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
