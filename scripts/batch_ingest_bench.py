"""How fast prompts enter batch slots, and what that costs the slots that are decoding: Gemma-2B Q4_0
(synthetic weights, the BASELINE config 2 shape), n_ctx 512, one engine, one process, eager launches
(the set-up of scripts/batch_bench.py).

    python scripts/batch_ingest_bench.py [--reps 3] [--prompt 128] [--legs ingest,arrival,wide]
                                         [--routes a,b,c] [--out FILE]
    python scripts/batch_ingest_bench.py --legs trace      (under rocprofv3 --kernel-trace --stats)

Every form is run once untimed first; the timed legs alternate `reps` times; medians with min - max.
  ingest   eight `prompt`-token prompts to their first generated token, begin to the last pass:
             a  batch_begin + batch_step(prompt): one token per pass and slot
             b  per slot begin; prefill; batch_adopt (through the engine's own sequence)
             c  open_rows(8, 64) + step_rows(64) until every prompt is consumed
           routes a and b use calls a build without step_rows has too (--routes a,b on such a build)
  arrival  16 slots decoding, then one `prompt`-token newcomer: its time to the first generated token
           and the decoders' tokens in that window, by b (the decoders wait) and by c (step_rows(64));
           each step_rows(64) pass's time beside batch_step at R = 16
  wide     batch_step at R = 64 (64 slots decoding), the pass the 64-row mixed pass is compared with
  trace    no timing: two 64-row mixed passes (16 decoders + 48 rows of a newcomer), then two batch_step
           passes at R = 64, so that a kernel trace holds k_rows_rope_kv / k_attn_slot_rows at T = 64
           and k_attn_slots at R = 64 from one session"""
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
ITERS = 24


def stats(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 1), min=round(v[0], 1), max=round(v[-1], 1), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--legs", default="ingest,arrival,wide")
    ap.add_argument("--routes", default="a,b,c")
    ap.add_argument("--out", default=None, help="also write the JSON summary to this file")
    args = ap.parse_args()
    legs, routes, P = args.legs.split(","), args.routes.split(","), args.prompt
    V = GEMMA_2B["n_vocab"]
    prompts = [[int(t) for t in make_prompt(P, V, seed=1 + s)] for s in range(64)]
    newcomer = [int(t) for t in make_prompt(P, V, seed=99)]
    e = G.Engine(GEMMA_2B, n_ctx=args.ctx)
    now = time.perf_counter
    res = {}

    def adopt(slot, prompt):
        e.begin(prompt)
        e.prefill(len(prompt))
        e.batch_adopt(slot)

    def rows_until(slot, target, times=None):
        """step_rows(64) passes until `slot` has consumed its given tokens; returns the pass count"""
        n = 0
        while e.batch_pos(slot) < target:
            t0 = now()
            e.batch_step_rows(64)
            if times is not None:
                times.append((now() - t0) * 1e6)
            n += 1
        return n

    if "ingest" in legs:
        def route_a():
            for s in range(8):
                e.batch_begin(s, prompts[s])
            e.batch_step(P)

        def route_b():
            for s in range(8):
                adopt(s, prompts[s])

        def route_c():
            for s in range(8):
                e.batch_begin(s, prompts[s])
            return rows_until(7, P)  # the budget is dealt in ascending slot order: slot 7 ends last

        run = dict(a=route_a, b=route_b, c=route_c)
        first = {}
        for rep in range(-1, args.reps):  # rep -1: every form once, untimed
            for r in routes:
                if r == "c":
                    e.batch_open_rows(8, 64)
                else:
                    e.batch_open(8)
                t0 = now()
                passes = run[r]()
                ms = (now() - t0) * 1e3
                # (by c a slot whose prompt is consumed decodes on while the later slots ingest)
                assert all(e.batch_pos(s) >= P if r == "c" else e.batch_pos(s) == P for s in range(8))
                toks = [int(e.batch_tokens(s)[P]) for s in range(8)]
                assert first.setdefault("tok", toks) == toks, (r, toks, first["tok"])  # the same first tokens by every route
                e.batch_close()
                if rep >= 0:
                    res.setdefault("ingest_" + r + "_ms", []).append(ms)
                    print(f"rep {rep} ingest {r}: {ms:8.2f} ms" + (f"  ({passes} passes)" if passes else ""), flush=True)

    if "arrival" in legs:
        e.batch_open_rows(17, 64)
        for s in range(16):
            adopt(s, prompts[s])
        e.batch_step(WARM)
        for rep in range(-1, args.reps):
            for r in ("b", "c"):
                t0 = now()
                e.batch_step(ITERS)
                us16 = (now() - t0) / ITERS * 1e6
                times = []
                t0 = now()
                if r == "b":
                    adopt(16, newcomer)
                    passes = 0
                else:
                    e.batch_begin(16, newcomer)
                    passes = rows_until(16, P, times)
                ms = (now() - t0) * 1e3
                assert e.batch_pos(16) == P
                e.batch_release(16)
                if rep >= 0:
                    res.setdefault("arrival_" + r + "_ttft_ms", []).append(ms)
                    res.setdefault("arrival_" + r + "_decoder_tokens", []).append(16 * passes)
                    res.setdefault("batch_step_R16_us", []).append(us16)
                    if times:
                        res.setdefault("step_rows_64_full_pass_us", []).extend(times[:-1])  # 16 + 48 rows
                        res.setdefault("step_rows_last_pass_us", []).append(times[-1])      # 16 + 32 rows
                    print(f"rep {rep} arrival {r}: newcomer first token after {ms:7.2f} ms, decoders made {16 * passes} tokens"
                          f" in it; batch_step R=16 {us16:7.1f} us/pass; row passes {[round(t) for t in times]}", flush=True)
        e.batch_close()

    if "wide" in legs:
        e.batch_open_rows(64, 64)
        for s in range(64):
            adopt(s, prompts[s])
        e.batch_step(WARM)
        for rep in range(args.reps):
            t0 = now()
            e.batch_step(ITERS)
            us = (now() - t0) / ITERS * 1e6
            res.setdefault("batch_step_R64_us", []).append(us)
            print(f"rep {rep} batch_step R=64 {us:7.1f} us/pass", flush=True)
        e.batch_close()

    if "trace" in legs:
        e.batch_open_rows(64, 64)
        for s in range(16):
            adopt(s, prompts[s])
        e.batch_begin(16, newcomer)
        for _ in range(2):
            rows_of, _ = e.batch_step_rows(64)
            assert int(rows_of.sum()) == 64 and rows_of[16] == 48, list(rows_of)
        e.batch_release(16)
        for s in range(16, 64):
            adopt(s, prompts[s])
        e.batch_step(2)
        e.batch_close()
        print("trace: 2 mixed passes of 64 rows, 2 batch_step passes at R = 64", flush=True)

    out = {k: stats(v) for k, v in res.items()}
    if "ingest_a_ms" in out and "ingest_c_ms" in out:
        out["c_max_below_a_min"] = bool(out["ingest_c_ms"]["max"] < out["ingest_a_ms"]["min"])
    line = json.dumps(dict(prompt=P, ctx=args.ctx, reps=args.reps, legs=legs, routes=routes, result=out))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
