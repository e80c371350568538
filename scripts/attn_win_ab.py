"""Decode step time near the end of a long context, resident against windowed split attention (option att_win).
argv: out.json.  A Gemma-2B-shaped Q4_0 engine at n_ctx 7904 (the last context the resident form serves at 8
heads per kv head): the prompt by prefill_next in chunks of 512, then windows of STEPS graph steps, att_win
0 1 1 0 0 1 (each after WARM steps that re-capture the graph), all within the last 300 positions.  Then the same
windows at n_ctx 8192, where only the windowed form runs.  step() returns after a device synchronise."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemma_hip as G  # noqa: E402
import oracle_ctypes as O  # noqa: E402

GEMMA_2B = dict(n_layer=18, n_embd=2048, n_head=8, n_head_kv=1, head_dim=256, n_ff=16384, n_vocab=256000)
WARM, STEPS = 6, 40


def windows(n_ctx, order):
    n_prompt = n_ctx - 1 - len(order) * (WARM + STEPS) - 4
    e = G.Engine(GEMMA_2B, n_ctx=n_ctx, device=0)
    e.begin(O.make_prompt(n_prompt, GEMMA_2B["n_vocab"]))
    while e.pos() < n_prompt:
        e.prefill_next(min(512, n_prompt - e.pos()))
    out = []
    for w in order:
        e.set_option("att_win", w)
        e.step(WARM, use_graph=True)
        p0 = e.pos()
        t0 = time.perf_counter()
        e.step(STEPS, use_graph=True)
        out.append(dict(att_win=w, first_pos=p0, us_per_token=(time.perf_counter() - t0) / STEPS * 1e6))
    e.close()
    return out


res = {"n_ctx_7904": windows(7904, [0, 1, 1, 0, 0, 1]), "n_ctx_8192": windows(8192, [0, 0, 0])}
print(json.dumps(res, indent=1))
with open(sys.argv[1], "w") as f:
    json.dump(res, f, indent=1)
