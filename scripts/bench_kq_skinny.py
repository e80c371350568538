#!/usr/bin/env python3
"""Times one gemma_engine_verify pass of T = 2, 3, 4, 6, 8 rows near position 256 on the synthetic
Gemma-2B Q4_K_M engine of bench.py --full's K-quant leg, for the three forms a skinny pass can take on
K-quant matrices: the T-column / MFMA kernels as dispatched without the option (kq_skinny 0), the MFMA
GEMM forced down to every T (hpc_set_kq_gemm_min(1)), and the skinny K-quant GEMM (kq_skinny 1).  The
contenders alternate inside each round; a pass is timed by the host clock around the call, which ends
in the device-to-host copy of the accepted tokens.  Prints one JSON line: per T and contender the
median over rounds of the per-round median pass time in ms, the min and max over rounds, and the
decode step time of the same engine as the unit.

    python scripts/bench_kq_skinny.py [--rounds 3] [--passes 12] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, ROOT)

import gemma_hip as G  # noqa: E402
from bench import GEMMA_2B, make_prompt  # noqa: E402

CONTENDERS = (("parent", 0, 8), ("mfma_min1", 0, 1), ("skinny_kq", 1, 8))  # name, kq_skinny, kq_gemm_min
TS = (2, 3, 4, 6, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--pos", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    V = GEMMA_2B["n_vocab"]
    prompt = make_prompt(args.pos, V)
    e = G.Engine(GEMMA_2B, n_ctx=args.pos + 256, wtype=G.GGML_TYPE_Q4_K, device=0)
    L = G.lib()

    def restart():
        e.begin(prompt)
        e.prefill(args.pos)

    restart()
    e.step(8, use_graph=True)
    e.sync()
    t0 = time.perf_counter()
    e.step(32, use_graph=True)
    e.sync()
    step_ms = (time.perf_counter() - t0) / 32 * 1e3
    per = {T: {c[0]: [] for c in CONTENDERS} for T in TS}
    for rnd in range(args.rounds + 1):  # round 0 warms every (contender, T) and is dropped
        for T in TS:
            for name, skinny, gmin in CONTENDERS:
                e.set_option("kq_skinny", skinny)
                L.hpc_set_kq_gemm_min(gmin)
                restart()
                ts = []
                for i in range(args.passes):
                    draft = [(7 * i + 3 * j + 11) % V for j in range(T - 1)]
                    t0 = time.perf_counter()
                    e.verify(draft)
                    ts.append((time.perf_counter() - t0) * 1e3)
                if rnd:
                    per[T][name].append(statistics.median(ts[2:]))
    L.hpc_set_kq_gemm_min(8)
    e.close()
    res = {"decode_step_ms": round(step_ms, 4), "pos": args.pos, "rounds": args.rounds, "passes": args.passes, "verify_ms": {}}
    for T in TS:
        res["verify_ms"][str(T)] = {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                    for n, v in per[T].items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
