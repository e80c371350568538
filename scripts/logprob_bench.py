"""What per-token log-probabilities cost: Gemma-2B Q4_0 (synthetic weights, bench.py's shape), one
process.

    python scripts/logprob_bench.py decode [--steps 512] [--reps 3] [--prompt 128]
    python scripts/logprob_bench.py score  [--T 2048] [--reps 3]
    python scripts/logprob_bench.py trace
    python scripts/logprob_bench.py table --csv <rocprofv3 ..._kernel_trace.csv>

decode  the scripts/sample_bench.py set-up: legs greedy / greedy+lp / k40 / k40+lp alternated `reps`
        times, each from the same state (begin, the prompt and 8 warm-up steps by graph replay, then
        `steps` timed graph replays with no host sync in between).  tok/s, us per token, launches.
score   a T-token text, three ways `reps` times after one warm-up round, their order rotating: `plain` the exact
        prefill alone; `device` the exact prefill with log-probabilities on and the T f64 values read
        back; `host` the exact prefill with logits_all copied to the host and the rule restated in
        numpy f64 there.  ms per way, the largest |device - host|, both perplexities.
trace   one call of every pass form with log-probabilities on, for `rocprofv3 --kernel-trace --stats`:
        R = 1 (8 decode steps), R = 8 (a verify pass of 7 drafts), R = 64 (a wide batch pass),
        R = 2048 (a prefill).  The k_lse_parts / k_lse_finish rows of the trace are the feature's time.
table   the k_lse_* launches of such a trace (and the decode logits launch beside them) by rows per
        launch: calls, min / median / max microseconds.
Prints one JSON line per mode (table: text)."""
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
V = GEMMA_2B["n_vocab"]


def stats(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2))


def decode(args):
    legs = [("greedy", None, 0), ("greedy+lp", None, 1), ("k40", K40, 0), ("k40+lp", K40, 1)]
    warm = 8
    e = G.Engine(GEMMA_2B, n_ctx=((args.prompt + warm + args.steps + 64) // 32 + 1) * 32)
    e.tune(8)
    prompt = make_prompt(args.prompt, V)
    us, launches = {k: [] for k, _, _ in legs}, {}
    for rep in range(args.reps):
        for name, smp, lp in legs:
            e.set_sampler(**smp) if smp else e.set_sampler(None)
            e.set_logprobs(lp)
            e.begin(prompt)
            e.step(args.prompt + warm, use_graph=True)
            e.sync()
            t0 = time.perf_counter()
            e.step(args.steps, use_graph=True)
            e.sync()
            dt = time.perf_counter() - t0
            us[name].append(dt / args.steps * 1e6)
            launches[name] = e.graph_kernels()
            scored = int(np.isfinite(e.logprobs(0, e.pos() + 1)).sum())
            print(f"rep {rep} {name:10s} {args.steps / dt:8.1f} tok/s {dt / args.steps * 1e6:7.1f} us/token "
                  f"launches/token {launches[name]} scored {scored}", flush=True)
    e.close()
    out = {k: dict(us_per_token=stats(v), tok_s_median=round(1e6 / stats(v)["median"], 1), launches_per_token=launches[k])
           for k, v in us.items()}
    out["added_us_per_token"] = {"greedy": round(out["greedy+lp"]["us_per_token"]["median"] - out["greedy"]["us_per_token"]["median"], 2),
                                 "k40": round(out["k40+lp"]["us_per_token"]["median"] - out["k40"]["us_per_token"]["median"], 2)}
    print(json.dumps(dict(mode="decode", steps=args.steps, reps=args.reps, prompt=args.prompt, legs=out)), flush=True)


def host_rule(rows, tokens):
    """lp of tokens[i + 1] under rows[i], i < len(rows) - 1: the rule in numpy f64, a block of rows at a time"""
    out = np.empty(len(rows) - 1)
    for r0 in range(0, len(out), 64):
        blk = rows[r0:min(r0 + 64, len(out))].astype(np.float64)
        blk -= blk.max(axis=1, keepdims=True)
        t = np.asarray(tokens[r0 + 1:r0 + 1 + len(blk)])
        out[r0:r0 + len(blk)] = blk[np.arange(len(blk)), t] - np.log(np.exp(blk).sum(axis=1))
    return out


def score(args):
    T = args.T
    e = G.Engine(GEMMA_2B, n_ctx=T + 64)
    text = [int(t) for t in make_prompt(T, V)]
    ms = {"plain": [], "device": [], "host": []}
    dev = host = None
    ways = ["plain", "device", "host"]
    for rep in range(args.reps + 1):  # the first round warms up (scratch, code objects) and is dropped
        # the order rotates: the leg behind `host` starts on a GPU that idled through seconds of numpy
        for way in ways[rep % 3:] + ways[:rep % 3]:
            e.set_logprobs(1 if way == "device" else 0)
            e.begin(text)
            e.sync()
            t0 = time.perf_counter()
            if way == "host":
                host = host_rule(e.prefill(T, want_all=True)[2], text)
            else:
                e.prefill(T)
                if way == "device":
                    dev = e.logprobs(1, T - 1)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ms[way].append(dt)
            print(f"rep {rep} {way:7s} {dt:10.2f} ms", flush=True)
    e.close()
    res = {k: stats(v) for k, v in ms.items()}
    print(json.dumps(dict(mode="score", T=T, reps=args.reps, ms=res,
                          added_over_plain_ms=round(res["device"]["median"] - res["plain"]["median"], 2),
                          max_abs_lp_diff=float(np.abs(dev - host).max()),
                          perplexity_device=float(np.exp(-dev.mean())), perplexity_host=float(np.exp(-host.mean())))), flush=True)


def trace(args):
    e = G.Engine(GEMMA_2B, n_ctx=512)
    e.set_logprobs(1)
    prompt = make_prompt(32, V)
    e.begin(prompt)
    e.prefill(32)
    e.step(8, use_graph=False)                       # R = 1, eight times
    e.verify([1, 2, 3, 4, 5, 6, 7])                  # R = 8
    e.batch_open_wide(64)
    for s in range(64):
        e.batch_begin(s, make_prompt(4, V, seed=s + 1) if s else prompt[:4])
    e.batch_step(1)                                  # R = 64
    e.batch_close()
    n = int(np.isfinite(e.logprobs(0, e.pos() + 1)).sum())
    e.close()
    e = G.Engine(GEMMA_2B, n_ctx=2048 + 64)
    e.set_logprobs(1)
    e.begin(make_prompt(2048, V))
    e.prefill(2048)                                  # R = 2048
    n2 = int(np.isfinite(e.logprobs(0, 2049)).sum())
    e.close()
    print(json.dumps(dict(mode="trace", scored_small=n, scored_prefill=n2)), flush=True)


def table(args):
    import collections
    import csv
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(args.csv)):
        n = r["Kernel_Name"]
        name = ("k_lse_parts" if "k_lse_parts" in n else "k_lse_finish" if "k_lse_finish" in n
                else "logits launch (k_matvec, argmax epilogue)" if "k_matvec<2, 1, 1, 3" in n else None)
        if name:
            key = (name, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]))
            acc[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("kernel | workgroups in x | rows (grid.y) | calls | us min | us median | us max")
    for k in sorted(acc):
        v = sorted(acc[k])
        print(" | ".join(str(x) for x in (k[0], k[1], k[2], len(v), round(v[0], 2), round(v[len(v) // 2], 2), round(v[-1], 2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["decode", "score", "trace", "table"])
    ap.add_argument("--csv")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--T", type=int, default=2048)
    args = ap.parse_args()
    {"decode": decode, "score": score, "trace": trace, "table": table}[args.mode](args)


if __name__ == "__main__":
    main()
