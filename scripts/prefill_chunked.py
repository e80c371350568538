"""Cost of feeding a prompt in pieces: the exact batched prefill of a T-token prompt in one pass
(Engine.prefill) against Engine.prefill_next in chunks, Gemma-2B Q4_0 shapes, one engine per mode so
that each mode's prefill scratch is its own.

usage: python scripts/prefill_chunked.py [T=2048] [modes=0,512,256] [reps=3] > profiles/<name>.json
(modes: chunk lengths, 0 = the one-pass prefill; a single mode serves a kernel trace of that mode)

Per mode: wall time of the whole prompt (host clock around calls that end in a stream synchronise;
the first repetition warms up and is dropped, the rest are listed), the prefill scratch in bytes
(computed from the shapes as prefill_alloc sizes it, and measured as the drop of free device memory
across the first pass), and whether the last row's logits and the greedy token equal the one-pass
prefill's bit for bit."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemma.ggml_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gemma_hip as G  # noqa: E402
import oracle_ctypes as O  # noqa: E402  (make_prompt only)


def free_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def scratch_bytes(shape, rows):
    """prefill_alloc(rows) for a Q4_0 / Q8_0 engine (csrc/engine_prefill.cpp)"""
    E, F, V = shape["n_embd"], shape["n_ff"], shape["n_vocab"]
    qw, kvw = shape["n_head"] * shape["head_dim"], shape["n_head_kv"] * shape["head_dim"]
    ldq = (max(E, F, qw) + 255) // 256 * 256
    per_row = (4 * (2 * E + (qw + 2 * kvw) + qw + 2 * F + V + ldq // 32)  # X SA QKV ATT G U LG DA
               + 2 * qw + ldq + 2 * ldq + (ldq // 256) * 32)             # Q16 XQ XH XM
    return rows * per_row + 256 * 8


def run(shape, prompt, chunk, reps):
    T = len(prompt)
    e = G.Engine(shape, n_ctx=T + 64, device=0)
    times, last, tok, before, used = [], None, None, free_bytes(), None
    for rep in range(reps + 1):
        e.begin(prompt)
        e.sync()
        t0 = time.perf_counter()
        if chunk is None:
            tok, last = e.prefill(T)
        else:
            while e.pos() < T:
                tok, last = e.prefill_next(min(chunk, T - e.pos()))
        times.append(time.perf_counter() - t0)
        if used is None:
            used = before - free_bytes()
    nxt = e.step(1, want_logits=True, use_graph=False)[0]  # the decode that reads the caches the passes wrote
    e.close()
    ms = [round(t * 1e3, 3) for t in times[1:]]
    return {"ms": ms, "ms_median": float(np.median(ms)), "scratch_bytes": scratch_bytes(shape, chunk or T),
            "device_memory_drop_bytes": used}, tok, last, nxt


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    modes = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "0,512,256").split(",")]
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    shape = dict(O.GEMMA_2B)
    prompt = O.make_prompt(T, shape["n_vocab"], seed=2)
    out = {"what": "exact batched prefill, Gemma-2B Q4_0 synthetic weights", "T": T, "reps": reps, "modes": {}}
    one = None
    for c in modes:
        r, tok, last, nxt = run(shape, prompt, c or None, reps)
        if c == 0:
            one, tok1, last1, nxt1 = r, tok, last, nxt
        else:
            r["passes"] = (T + c - 1) // c
        if c and one:
            r["vs_one_pass"] = round(r["ms_median"] / one["ms_median"], 3)
            r["same_bits_as_one_pass"] = bool(tok == tok1 and np.array_equal(last.view(np.uint32), last1.view(np.uint32))
                                              and np.array_equal(nxt.view(np.uint32), nxt1.view(np.uint32)))
        out["modes"][f"chunks_of_{c}" if c else "one_pass"] = r
    print(json.dumps(out, indent=1))
    if not all(m.get("same_bits_as_one_pass", True) for m in out["modes"].values()):
        sys.exit("chunked prefill differs from the one-pass prefill")


if __name__ == "__main__":
    main()
