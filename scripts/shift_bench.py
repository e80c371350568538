#!/usr/bin/env python3
"""What a context shift costs beside what it replaces (DESIGN.md §5b′ "Context shift").

Gemma-2B Q4_0, synthetic weights, n_ctx 8192.  At pos 8,190: one gemma_engine_shift(keep 32, discard D) for D in
1,024 and 4,096 (host clock around the call, which ends in a synchronise; median and range of --reps calls, the
sequence refilled to 8,190 in between), one decode step at positions 8,182 .. 8,189 through the captured graph, and
the exact prefill of pos - D tokens from position 0 in passes of 512 (gemma_engine_prefill_next), the only way to
the same state without the shift.  Bytes: the algorithm's, from the shapes: per cache and layer the moved span is
read once and span + D positions are written once.  One JSON object on stdout, or into --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemma_hip as G  # noqa: E402
import oracle_ctypes as O  # noqa: E402

GEMMA_2B = dict(n_layer=18, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=16384, n_vocab=256000)
N_CTX, POS, KEEP, CHUNK = 8192, 8190, 32, 512


def prefill_all(e):
    while e.pos() < e._n_seq:
        e.prefill_next(min(CHUNK, e._n_seq - e.pos()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V = GEMMA_2B["n_vocab"]
    toks = [int(t) for t in O.make_prompt(N_CTX, V)]
    e = G.Engine(GEMMA_2B, n_ctx=N_CTX, device=0)
    res = dict(model="gemma-2b q4_0 synthetic", n_ctx=N_CTX, pos=POS, keep=KEEP, reps=a.reps)
    # the prefill a shift replaces: pos - D tokens from position 0
    e.begin(toks[:CHUNK])
    prefill_all(e)  # warm-up: code objects, scratch
    for D in (1024, 4096):
        ts = []
        for _ in range(3):
            e.begin(toks[:POS - D])
            t0 = time.perf_counter()
            prefill_all(e)
            e.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[f"prefill_{POS - D}_ms"] = dict(median=statistics.median(ts), min=min(ts), max=max(ts))
    # one decode step near the end of the context, graph replay
    e.begin(toks[:POS - 10])
    prefill_all(e)
    e.step(2, use_graph=True)
    t0 = time.perf_counter()
    e.step(8, use_graph=True)
    res["decode_step_us"] = (time.perf_counter() - t0) * 1e6 / 8
    assert e.pos() == POS
    kvw, L = GEMMA_2B["n_head_kv"] * GEMMA_2B["head_dim"], GEMMA_2B["n_layer"]
    for D in (1024, 4096):
        ts = []
        for rep in range(a.reps + 1):  # the first call is the warm-up
            assert e.pos() == POS
            t0 = time.perf_counter()
            e.shift(KEEP, D)
            ts.append((time.perf_counter() - t0) * 1e6)
            e.extend(toks[:D - 1])  # the pending token and D - 1 more: back to POS
            prefill_all(e)
        ts = ts[1:]
        span = POS - KEEP - D
        nbytes = 2 * L * kvw * 2 * (span + span + D)  # K and V: the span read, span + D positions written
        med = statistics.median(ts)
        res[f"shift_{D}"] = dict(us_median=med, us_min=min(ts), us_max=max(ts), bytes=nbytes, gb_per_s=nbytes / med * 1e-3)
    e.close()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
